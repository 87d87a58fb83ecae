"""The CenterPoint second stage (inference): ``TwoStageDetector``, ``BEVFeatureExtractor`` and ``RoIHead`` under the reference's names.

Reference: det3d/models/detectors/two_stage.py:8-193, det3d/models/second_stage/bird_eye_view.py:9-41,
det3d/models/roi_heads/roi_head.py:16-106, roi_head_template.py:18-41, 153-183.

The first stage leaves its detections on the device (``CenterHead.predict(device_only=True)``: fixed-capacity buffers and counts) and its
neck output is NHWC already, so the second stage is `pn_roi_bev_gather_f32` -> the RoIHead's token GEMMs -> `pn_roi_refine_f32`: no
per-sample Python loop, nothing read back, capturable in a hipGraph.  f32, eval mode.  Training of the second stage on a frozen first stage
has a surface of its own, ``train_two_stage.TwoStageTrainStep`` (proposal targets in roi_targets.py); ``forward(return_loss=True)``,
``RoIHead.forward(training=True)`` and ``RoIHead.get_loss`` keep refusing.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List

import torch
from torch import nn

from . import builder, hip
from .builder import DETECTORS, ROI_HEAD, SECOND_STAGE
from .nn_utils import PlanCache, eval_only
from .ops_token import ACT_NONE, ACT_RELU, GemmLayer

DEVICE_LIST_KEYS = ("box3d_lidar", "scores", "label_preds")


def _get(cfg, key, default=None):
    """a value of a dict or of an attribute dict"""
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


@SECOND_STAGE.register_module
class BEVFeatureExtractor(nn.Module):
    """bird_eye_view.py:9-41: per ROI the bilinear samples of the BEV map at the box centre (and the four face midpoints).  No parameters.
    ``forward`` is the fused launch: get_box_center + the samples + the zero-padded, reordered ROI buffers of two_stage.py:78-119."""

    def __init__(self, pc_start, voxel_size, out_stride):
        super().__init__()
        self.pc_start = pc_start
        self.voxel_size = voxel_size
        self.out_stride = out_stride

    def forward(self, dets: Dict[str, torch.Tensor], bev: torch.Tensor, num_point: int, code_size: int, max_rois: int) -> Dict[str, torch.Tensor]:
        """dets: the first stage's device list ('box3d_lidar' (B, cap, 7|9), 'scores', 'label_preds' int64, 'count' int32; rows at or past
        the count are never read); bev: the NHWC map (B, H, W, C), possibly a channel slice of a wider map.
        -> 'rois' (B, max_rois, code_size), 'roi_scores', 'roi_labels' (= label + 1), 'roi_features' (B, max_rois, num_point * C), 'count';
        slots at or past the count are zeros."""
        boxes, scores, labels, count = dets["box3d_lidar"], dets["scores"], dets["label_preds"], dets["count"]
        hip.require_device(boxes, scores, labels, count, bev)
        b, cap, cols = boxes.shape
        assert boxes.dtype == torch.float32 and boxes.is_contiguous() and scores.dtype == torch.float32 and scores.is_contiguous()
        assert labels.dtype == torch.int64 and labels.is_contiguous() and count.dtype == torch.int32 and count.is_contiguous()
        assert tuple(scores.shape) == (b, cap) and tuple(labels.shape) == (b, cap) and tuple(count.shape) == (b,)
        assert bev.dim() == 4 and bev.dtype == torch.float32 and bev.shape[0] == b
        _, h, w, c = bev.shape
        ps = bev.stride(2)
        if not (bev.stride(3) == 1 and bev.stride(1) == w * ps and (b == 1 or bev.stride(0) == h * w * ps)):
            raise hip.PartnerHipError("BEVFeatureExtractor: the map must be an NHWC tensor or a channel slice of one")
        dev = boxes.device
        out = dict(rois=torch.empty((b, max_rois, code_size), dtype=torch.float32, device=dev),
                   roi_scores=torch.empty((b, max_rois), dtype=torch.float32, device=dev),
                   roi_labels=torch.empty((b, max_rois), dtype=torch.int64, device=dev),
                   roi_features=torch.empty((b, max_rois, num_point * c), dtype=torch.float32, device=dev), count=count)
        hip.call("pn_roi_bev_gather_f32", boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), count.data_ptr(), b, cap, cols,
                 bev.data_ptr(), h, w, c, ps, (C.c_float * 2)(*[float(v) for v in self.pc_start[:2]]),
                 (C.c_float * 2)(*[float(v) for v in self.voxel_size[:2]]), int(self.out_stride), int(num_point), int(code_size), int(max_rois),
                 out["rois"].data_ptr(), out["roi_scores"].data_ptr(), out["roi_labels"].data_ptr(), out["roi_features"].data_ptr(),
                 num_point * c, hip.stream())
        return out


def _fold_conv_bn(conv: nn.Conv1d, bn: nn.BatchNorm1d):
    """Conv1d(k = 1, no bias) + eval BatchNorm1d -> the rows and bias of one GEMM (folded in float64, rounded once)"""
    w = conv.weight.detach().double()[:, :, 0]
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return (w * scale[:, None]).float(), (bn.bias.detach().double() - bn.running_mean.detach().double() * scale).float()


def _branch(seq: nn.Sequential):
    """a Sequential of make_fc_layers / the shared layers -> ([(weight, bias) of every Conv1d + BatchNorm1d pair], the final biased Conv1d or None)"""
    mods, pairs, final = list(seq), [], None
    for i, m in enumerate(mods):
        if isinstance(m, nn.Conv1d):
            if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d):
                pairs.append(_fold_conv_bn(m, mods[i + 1]))
            else:
                final = m
    return pairs, final


def _gemm(layer: GemmLayer, x: torch.Tensor, x_col: int, out: torch.Tensor, out_col: int, act: int):
    """``layer`` on the columns [x_col, x_col + k) of the row buffer x, into the columns [out_col, out_col + n) of the row buffer out
    (``GemmLayer.__call__`` takes and returns whole contiguous matrices; the entry itself takes row strides)"""
    assert x.dim() == 2 and out.dim() == 2 and x.is_contiguous() and out.is_contiguous() and x.shape[0] == out.shape[0]
    assert x_col % 4 == 0 and out_col % 4 == 0 and x_col + layer.k <= x.shape[1] and out_col + layer.n <= out.shape[1]
    hip.call(layer.entry, x.data_ptr() + 4 * x_col, x.shape[0], layer.k, x.shape[1], layer.packed.data_ptr(), layer.n, hip.ptr(layer.bias), int(act),
             None, layer.n, out.data_ptr() + 4 * out_col, out.shape[1], hip.stream())


@ROI_HEAD.register_module
class RoIHead(nn.Module):
    """roi_head.py:16-106 (inference): shared MLP -> a classification and a regression branch, every layer a 1x1 Conv1d (+ BatchNorm1d +
    ReLU).  The modules are built as the reference builds them (the Dropout entries shift the indices), so its checkpoints load strictly.
    Eval plan: every Conv1d + BatchNorm1d pair is one GemmLayer with the statistics folded in; cls_layers[0] and reg_layers[0] read the same
    rows and run as ONE GEMM; the two final layers write one (rows, 4 + pad4(code_size)) buffer (``rcnn_rows``), which
    `pn_roi_refine_f32` reads by column offset."""

    CLS_COL, REG_COL = 0, 4      # columns of rcnn_cls / rcnn_reg in the final row buffer

    def __init__(self, input_channels, model_cfg, num_class=1, code_size=7, test_cfg=None):
        super().__init__()
        self.model_cfg, self.num_class, self.test_cfg, self.code_size = model_cfg, num_class, test_cfg, code_size
        shared, dp = list(_get(model_cfg, "SHARED_FC")), _get(model_cfg, "DP_RATIO")
        pre_channel, layers = input_channels, []
        for k, width in enumerate(shared):
            layers.extend([nn.Conv1d(pre_channel, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()])
            pre_channel = width
            if k != len(shared) - 1 and dp > 0:
                layers.append(nn.Dropout(dp))
        self.shared_fc_layer = nn.Sequential(*layers)
        self.cls_layers = self.make_fc_layers(pre_channel, self.num_class, list(_get(model_cfg, "CLS_FC")))
        self.reg_layers = self.make_fc_layers(pre_channel, code_size, list(_get(model_cfg, "REG_FC")))
        self.init_weights(weight_init="xavier")
        self._plan = PlanCache()

    def make_fc_layers(self, input_channels, output_channels, fc_list):
        """roi_head_template.py:27-41"""
        layers, pre_channel, dp = [], input_channels, _get(self.model_cfg, "DP_RATIO")
        for k, width in enumerate(fc_list):
            layers.extend([nn.Conv1d(pre_channel, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()])
            pre_channel = width
            if dp >= 0 and k == 0:
                layers.append(nn.Dropout(dp))
        layers.append(nn.Conv1d(pre_channel, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*layers)

    def init_weights(self, weight_init="xavier"):
        """roi_head.py:50-68"""
        funcs = dict(kaiming=nn.init.kaiming_normal_, xavier=nn.init.xavier_normal_, normal=nn.init.normal_)
        if weight_init not in funcs:
            raise NotImplementedError(weight_init)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                if weight_init == "normal":
                    nn.init.normal_(m.weight, mean=0, std=0.001)
                else:
                    funcs[weight_init](m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    # -- the eval plan -------------------------------------------------------------------------
    def _build_plan(self):
        if self.num_class != 1:
            raise NotImplementedError("RoIHead: num_class != 1 (post_process multiplies ONE class-agnostic score per ROI, two_stage.py:134)")
        dev = next(self.parameters()).device
        shared, _ = _branch(self.shared_fc_layer)
        (cls, cls_final), (reg, reg_final) = _branch(self.cls_layers), _branch(self.reg_layers)
        merged = None

        def gemm(w, b):      # B * NMS_POST_MAXSIZE rows (500 - 1000 in the reference's configs): the K-split form of the token GEMM, measured
            return GemmLayer(w.to(dev), b.to(dev), ksplit=True)      # at 43 - 52 us for the seven layers against 76 - 86 us tiled
        if cls and reg:      # both branches start on the shared features: one GEMM with the output columns side by side
            merged = (gemm(torch.cat([cls[0][0], reg[0][0]]), torch.cat([cls[0][1], reg[0][1]])), cls[0][0].shape[0])
            cls, reg = cls[1:], reg[1:]

        def final(conv, rows):      # the biased last Conv1d, its rows zero-padded to a multiple of 4 (the GEMM's n % 4 == 0)
            w = torch.zeros((rows, conv.in_channels), dtype=torch.float32, device=dev)
            b = torch.zeros((rows,), dtype=torch.float32, device=dev)
            w[:conv.out_channels] = conv.weight.detach()[:, :, 0]
            b[:conv.out_channels] = conv.bias.detach()
            return gemm(w, b)
        plan = dict(shared=[gemm(w, b) for w, b in shared], merged=merged, cls=[gemm(w, b) for w, b in cls], reg=[gemm(w, b) for w, b in reg],
                    cls_final=final(cls_final, 4), reg_final=final(reg_final, _pad4(self.code_size)))
        for layer in plan["shared"] + plan["cls"] + plan["reg"] + ([merged[0]] if merged else []) + [plan["cls_final"], plan["reg_final"]]:
            if layer.k % 4 or layer.n % 4 or (merged and merged[1] % 4):
                raise ValueError("RoIHead: the input channels and every SHARED_FC / CLS_FC / REG_FC width must be multiples of 4 "
                                 "(16-byte rows of the token GEMM)")
        return plan

    def rcnn_rows(self, roi_features: torch.Tensor) -> torch.Tensor:
        """roi_head.py:83-91 on (rows, input_channels) features -> the (rows, 4 + pad4(code_size)) buffer that holds rcnn_cls in column
        CLS_COL and rcnn_reg in columns [REG_COL, REG_COL + code_size)"""
        eval_only(self, "RoIHead")
        hip.require_device(roi_features)
        assert roi_features.dim() == 2 and roi_features.dtype == torch.float32 and roi_features.is_contiguous()
        plan = self._plan.get(self, self._build_plan)
        m, dev = roi_features.shape[0], roi_features.device

        def run(layers, x, col):
            for layer in layers:
                y = torch.empty((m, layer.n), dtype=torch.float32, device=dev)
                _gemm(layer, x, col, y, 0, ACT_RELU)
                x, col = y, 0
            return x, col
        x, _ = run(plan["shared"], roi_features, 0)
        cls_in, reg_in = (x, 0), (x, 0)
        if plan["merged"] is not None:
            layer, split = plan["merged"]
            y = torch.empty((m, layer.n), dtype=torch.float32, device=dev)
            _gemm(layer, x, 0, y, 0, ACT_RELU)
            cls_in, reg_in = (y, 0), (y, split)
        out = torch.empty((m, self.REG_COL + _pad4(self.code_size)), dtype=torch.float32, device=dev)
        _gemm(plan["cls_final"], *run(plan["cls"], *cls_in), out, self.CLS_COL, ACT_NONE)
        _gemm(plan["reg_final"], *run(plan["reg"], *reg_in), out, self.REG_COL, ACT_NONE)
        return out

    def forward(self, batch_dict, training=True):
        """batch_dict: what ``BEVFeatureExtractor.forward`` returned.  Adds 'rcnn_cls' (rows, 1) and 'rcnn_reg' (rows, code_size) -- views of
        one row buffer -- and 'det': the refined device list in the first stage's format ('box3d_lidar' (B, max_rois, code_size) in the
        head's column order, 'scores' = sqrt(sigmoid(rcnn_cls) * roi_score), 'label_preds', 'count'; rows at or past the count are zeros)."""
        if training:
            raise NotImplementedError("RoIHead.forward(training=True) is not built: the ProposalTargetLayer samples ROIs at random by 3-D IoU from a "
                                      "CUDA-only op, so the second stage's training has no CPU reference to pin it to; call forward(batch_dict, training=False)")
        rois, scores, labels, count = batch_dict["rois"], batch_dict["roi_scores"], batch_dict["roi_labels"], batch_dict["count"]
        b, r, cs = rois.shape
        assert cs == self.code_size, f"RoIHead: rois have {cs} columns, code_size is {self.code_size}"
        rows = self.rcnn_rows(batch_dict["roi_features"].reshape(b * r, -1))
        dev = rois.device
        det = dict(box3d_lidar=torch.empty((b, r, cs), dtype=torch.float32, device=dev), scores=torch.empty((b, r), dtype=torch.float32, device=dev),
                   label_preds=torch.empty((b, r), dtype=torch.int64, device=dev), count=torch.empty((b,), dtype=torch.int32, device=dev))
        hip.call("pn_roi_refine_f32", rois.data_ptr(), scores.data_ptr(), labels.data_ptr(), count.data_ptr(), b, r, cs, rows.data_ptr(), rows.shape[1],
                 self.CLS_COL, rows.data_ptr(), rows.shape[1], self.REG_COL, det["box3d_lidar"].data_ptr(), det["scores"].data_ptr(),
                 det["label_preds"].data_ptr(), det["count"].data_ptr(), hip.stream())
        batch_dict["batch_size"] = b
        batch_dict["rcnn_cls"], batch_dict["rcnn_reg"] = rows[:, self.CLS_COL:self.CLS_COL + 1], rows[:, self.REG_COL:self.REG_COL + cs]
        batch_dict["det"] = det
        return batch_dict

    def get_loss(self, tb_dict=None):
        raise NotImplementedError("RoIHead.get_loss is not built: the ProposalTargetLayer samples ROIs at random by 3-D IoU from a CUDA-only op, "
                                  "so the second stage's training has no CPU reference to pin it to")


@DETECTORS.register_module
class TwoStageDetector(nn.Module):
    """two_stage.py:8-193 (inference): a first stage built from ``first_stage_cfg`` (PointPillars or VoxelNet with one CenterHead task), the
    BEV feature gather and the RoIHead refinement of its detections.  ``bbox_head`` is the reference's alias of ``single_det.bbox_head``
    (its state_dict carries both sets of keys)."""

    def __init__(self, first_stage_cfg, second_stage_modules, roi_head, NMS_POST_MAXSIZE, num_point=1, freeze=False, **kwargs):
        super().__init__()
        self.single_det = builder.build_detector(first_stage_cfg, **kwargs)
        self.NMS_POST_MAXSIZE = int(NMS_POST_MAXSIZE)
        self.freeze = bool(freeze)
        if freeze:      # the reference trains in two steps: the first stage stays as it was trained
            self.single_det.eval()
            self.single_det.requires_grad_(False)
        self.bbox_head = self.single_det.bbox_head
        self.second_stage = nn.ModuleList()
        for module in second_stage_modules:
            kind = _get(module, "type")
            if kind != "BEVFeatureExtractor":
                raise NotImplementedError(f"TwoStageDetector: second-stage module {kind} is not built; BEVFeatureExtractor is")
            self.second_stage.append(builder.build_second_stage_module(module))
        if len(self.second_stage) != 1:
            raise NotImplementedError(f"TwoStageDetector: {len(self.second_stage)} second-stage modules; exactly one BEVFeatureExtractor is built "
                                      "(the voxel_feature stream of two_stage.py:157-159 and further streams are not)")
        self.roi_head = builder.build_roi_head(roi_head)
        self.num_point = int(num_point)
        self.test_cfg = kwargs.get("test_cfg")
        self._refuse_unbuilt(False)

    def train(self, mode: bool = True):
        """under ``freeze`` the first stage stays in eval form (the reference's ``SingleStageDetector.freeze`` turns its BatchNorms into
        frozen ones, which ``train()`` does not touch)"""
        super().train(mode)
        if self.freeze:
            self.single_det.eval()
        return self

    def set_compute_dtype(self, dtype: str):
        if dtype != "f32":
            raise NotImplementedError(f"TwoStageDetector runs in f32 only: {dtype} is not built for the ROI kernels and the RoIHead's GEMMs")
        return self

    def _refuse_unbuilt(self, return_loss):
        if return_loss:
            raise NotImplementedError("TwoStageDetector: return_loss=True is not built (the second stage runs inference only: RoIHead.get_loss "
                                      "says why); call forward(example, return_loss=False)")
        if not hasattr(self.single_det, "forward_two_stage"):
            raise NotImplementedError(f"TwoStageDetector: a {type(self.single_det).__name__} first stage has no forward_two_stage; PointPillars and VoxelNet have")
        if self.bbox_head is None or len(self.bbox_head.tasks) != 1:
            raise NotImplementedError("TwoStageDetector: a first stage with more than one task is not built (the device list holds one task)")
        cfg = self.test_cfg
        if cfg is None:
            return
        for flag in ("double_flip", "stateful_nms", "panoptic"):
            if bool(_get(cfg, flag, False)):
                raise NotImplementedError(f"TwoStageDetector: test_cfg.{flag} in front of the second stage is not built")
        post = int(_get(_get(cfg, "nms"), "nms_post_max_size"))
        if post > self.NMS_POST_MAXSIZE:
            raise ValueError(f"TwoStageDetector: test_cfg.nms.nms_post_max_size = {post} exceeds NMS_POST_MAXSIZE = {self.NMS_POST_MAXSIZE}: the ROI "
                             "buffers could not hold the first stage's boxes")

    def second_stage_device(self, dets: Dict[str, torch.Tensor], bev: torch.Tensor) -> Dict[str, torch.Tensor]:
        """the first stage's device list + its NHWC neck output -> the refined device list (gather, RoIHead GEMMs, refine)"""
        batch = self.second_stage[0](dets, bev, self.num_point, self.roi_head.code_size, self.NMS_POST_MAXSIZE)
        return self.roi_head(batch, training=False)["det"]

    @torch.no_grad()
    def forward(self, example, return_loss=False, device_only=False, **kwargs):
        """-> the reference's list of per-sample dicts ('box3d_lidar', 'scores', 'label_preds', 'metadata'), cut with ONE readback of the
        counts; ``device_only=True``: the device list itself ('box3d_lidar' (B, NMS_POST_MAXSIZE, 7|9), 'scores', 'label_preds', 'count'),
        nothing read back (``to_host`` cuts it later)"""
        self._refuse_unbuilt(return_loss)
        dets, bev = self.single_det.forward_two_stage(example, return_loss, **kwargs)
        out = self.second_stage_device(dets, bev)
        return out if device_only else self.to_host(out, example)

    @staticmethod
    def to_host(out: Dict[str, torch.Tensor], example) -> List[dict]:
        """the result of ``forward(..., device_only=True)`` -> exactly what ``forward(...)`` returns; ONE readback, of the counts"""
        counts = out["count"].tolist()
        metas = example.get("metadata", [None] * len(counts)) if isinstance(example, dict) else [None] * len(counts)
        res = []
        for i, n in enumerate(counts):
            d = {k: out[k][i, :n] for k in DEVICE_LIST_KEYS}
            d["metadata"] = metas[i]
            res.append(d)
        return res
