"""Segmentation head of the reference's nuScenes polar config (`super_tasks = ['det', 'seg']`): SingleConvHead
(det3d/models/seg_heads/seg_head.py:53-83, 99-168, 176-195) and its loss object SegLoss (det3d/models/losses/seg_loss.py:8-22).
Secondary to the detection hot path: forward, per-point prediction and the panoptic fusion with the detection boxes run on the HIP
kernels (eval); the loss (Lovasz softmax + cross entropy) is not built."""
from __future__ import annotations

import math

import torch
from torch import nn

from . import builder, hip, ops
from .builder import LOSSES, SEG_HEAD
from .nn_utils import PlanCache, eval_only

# the ten nuScenes lidarseg thing classes in label order (semantic labels 1..10) under their detection class names
# (the module constant `semantic2box`, seg_head.py:11-22)
SEMANTIC2BOX = ["barrier", "bicycle", "bus", "car", "construction_vehicle", "motorcycle", "pedestrian", "traffic_cone", "trailer", "truck"]


@LOSSES.register_module
class SegLoss(nn.Module):
    """parameter-free; kept so that the config's ``loss=dict(type='SegLoss', ignore=-1)`` builds"""

    def __init__(self, ignore=0):
        super().__init__()
        self.ignore = ignore

    def forward(self, outputs, labels):
        raise NotImplementedError("SegLoss (Lovasz softmax + cross entropy, seg_loss.py:19-22) is not built: segmentation training is out of scope")


@SEG_HEAD.register_module
class SingleConvHead(nn.Module):
    """seg_preds = Conv2d(in_channels, num_classes, kernel)(cat[x1, bilinear_up(x2 -> size of x1)]), x1 = BEV canvas, x2 = RPN output.

    With the config's kernel = 1 the convolution commutes with the interpolation, so the head runs as
    conv(x1; W[:, :C1]) + bias + bilinear_up(conv(x2; W[:, C1:])) and the (C1 + C2)-channel map at canvas resolution is never built."""

    def __init__(self, kernel=1, num_classes=16, in_channels=448, weight=1, loss=None):
        super().__init__()
        self.num_classes = num_classes
        self.conv = nn.Conv2d(in_channels, num_classes, kernel, padding=kernel // 2)
        self.weight = weight
        self.loss_func = builder.build_loss(loss) if loss is not None else None
        self._plan = PlanCache()

    def _build_plan(self, c1: int):
        if self.conv.kernel_size != (1, 1):
            raise NotImplementedError("SingleConvHead: only kernel=1 (the reference config) has a HIP path")
        w = self.conv.weight
        n = self.num_classes
        npad = (n + 3) // 4 * 4                      # the up-sampling kernel moves 16-byte channel groups
        wa = torch.zeros((npad, c1, 1, 1), dtype=w.dtype, device=w.device)
        wb = torch.zeros((npad, w.shape[1] - c1, 1, 1), dtype=w.dtype, device=w.device)
        bias = torch.zeros((npad,), dtype=w.dtype, device=w.device)
        wa[:n], wb[:n], bias[:n] = w[:, :c1].detach(), w[:, c1:].detach(), self.conv.bias.detach()
        return dict(c1=c1, npad=npad, a=ops.ConvLayer(wa, shift=bias, act=ops.ACT_NONE), b=ops.ConvLayer(wb, act=ops.ACT_NONE))

    def forward_nhwc(self, x1: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
        """x1 (B,H,W,C1), x2 (B,h,w,C2) NHWC -> logits (B,H,W,num_classes [padded to a multiple of 4]) NHWC"""
        hip.require_device(x1, x2)
        eval_only(self, "SingleConvHead")
        plan = self._plan.get(self, lambda: self._build_plan(x1.shape[3]))
        assert plan["c1"] == x1.shape[3] and x1.shape[3] + x2.shape[3] == self.conv.in_channels, "channel split does not match in_channels"
        out = plan["a"](x1)
        low = plan["b"](x2)
        b, h, w, c = low.shape
        hip.call("pn_bilinear_upsample_add_f32", low.data_ptr(), b, h, w, c, out.shape[1], out.shape[2], out.data_ptr(), hip.stream())
        return out

    def forward(self, x1, x2):
        """logical (B,C,H,W) tensors, as seg_head.py:75-83 -> {'seg_preds': (B, num_classes, H, W)}"""
        out = self.forward_nhwc(ops.to_nhwc(x1), ops.to_nhwc(x2))
        return {"seg_preds": out.permute(0, 3, 1, 2)[:, :self.num_classes]}

    def loss(self, example, preds_dicts, **kwargs):
        raise NotImplementedError("SingleConvHead.loss: segmentation training is out of scope (SegLoss is not built)")

    @torch.no_grad()
    def predict(self, example, preds_dicts, test_cfg, **kwargs):
        """per-point semantic labels (seg_head.py:176-195): 1 + argmax over the classes at every point's BEV cell
        (``example['valid_grid_ind'][i]``: (n_i, 3) [z, y, x]).  -> list of {token: labels (n_i,) int64}"""
        seg = preds_dicts["seg_preds"]
        hip.require_device(seg)
        assert seg.dim() == 4 and seg.stride(1) == 1, "seg_preds must be the channels-last view produced by forward"
        bsz, ncls, h, w = seg.shape
        cstride = seg.stride(3)                                  # padded channel count of the NHWC buffer
        if kwargs.get("device_only", False):
            # one launch for the sector, nothing read back: -> flat (rows,) int64, one label per point row in row order
            gi, offs = self._flat_rows(example, seg.device)
            labels = torch.empty((gi.shape[0],), dtype=torch.int64, device=seg.device)
            self._launch_batched(seg, gi, offs, labels)
            return labels
        out = []
        for i in range(bsz):
            gi = example["valid_grid_ind"][i]
            gi = (gi if torch.is_tensor(gi) else torch.as_tensor(gi)).to(seg.device).to(torch.int64).contiguous()
            labels = torch.empty((gi.shape[0],), dtype=torch.int64, device=seg.device)
            # the kernel reads `classes` logits with the buffer's pixel stride: pass the sample's base pointer and the real class count
            base = seg[i].permute(1, 2, 0)                       # (H, W, ncls) view, pixel stride = cstride
            assert base.stride(2) == 1 and base.stride(1) == cstride
            if cstride != ncls:                                  # padded buffer: compact once (small: H*W*ncls floats)
                base = base.contiguous()
            if gi.shape[0]:                                      # a sample without points in this sector (streaming): an empty label tensor
                hip.call("pn_seg_point_labels", base.data_ptr(), h, w, ncls, gi.data_ptr(), gi.shape[0], labels.data_ptr(), hip.stream())
            meta = example["metadata"][i]
            token = meta["token"] if isinstance(meta, dict) and "token" in meta else i
            out.append({token: labels})
        return out

    @staticmethod
    def _flat_rows(example, dev):
        """device_only inputs: the sector's grid indices as ONE (rows, 3) int64 tensor (``example['valid_grid_ind']``: that tensor, or the
        per-sample list, concatenated on the device) and the samples' row offsets, device int32 (B + 1,): ``example['point_offsets']``
        when present, otherwise built once from the host ``num_points`` and kept in the example (an upload: not capturable)"""
        gi = example["valid_grid_ind"]
        if not torch.is_tensor(gi):
            hip.require_device(*gi)
            gi = torch.cat([g.to(torch.int64) for g in gi], 0) if len(gi) > 1 else gi[0]
        hip.require_device(gi)
        gi = gi.to(torch.int64).contiguous()
        assert gi.dim() == 2 and gi.shape[1] == 3, "valid_grid_ind must hold one [z, y, x] row per point"
        offs = example.get("point_offsets")
        if offs is None:
            num = example["num_points"]
            num = [int(v) for v in (num.tolist() if torch.is_tensor(num) else num)]
            assert sum(num) <= gi.shape[0], "num_points does not match valid_grid_ind"
            acc = [0]
            for v in num:
                acc.append(acc[-1] + v)
            offs = example["point_offsets"] = torch.tensor(acc, dtype=torch.int32, device=dev)
        hip.require_device(offs)
        assert offs.dtype == torch.int32 and offs.dim() == 1 and offs.is_contiguous(), "point_offsets must be a contiguous int32 (B + 1,) tensor"
        return gi, offs

    def _launch_batched(self, seg, gi, offs, labels, points=None, x_col=0, angle=0.0, det=None, sem2box=None, score_thr=0.0, ins=None):
        """`pn_panoptic_points_batched_f32` on the (possibly channel-padded) NHWC logits, read in place; det None: labels only"""
        bsz, ncls, h, w = seg.shape
        assert offs.shape[0] == bsz + 1, "point_offsets must have one entry per sample plus one"
        assert seg.stride(2) == w * seg.stride(3) and (bsz == 1 or seg.stride(0) >= h * w * seg.stride(3))
        if det is None:
            hip.call("pn_panoptic_points_batched_f32", seg.data_ptr(), seg.stride(0) if bsz > 1 else 0, bsz, h, w, ncls, seg.stride(3), gi.data_ptr(),
                     offs.data_ptr(), gi.shape[0], None, 0, 0, 1.0, 0.0, None, 0, 0, None, None, None, None, None, 0.0, labels.data_ptr(), None, hip.stream())
            return
        boxes = det["box3d_lidar"]
        cap = int(boxes.shape[1])
        point_stride = points.stride(0) if points.shape[0] > 1 else points.shape[1]
        hip.call("pn_panoptic_points_batched_f32", seg.data_ptr(), seg.stride(0) if bsz > 1 else 0, bsz, h, w, ncls, seg.stride(3), gi.data_ptr(),
                 offs.data_ptr(), gi.shape[0], points.data_ptr(), point_stride, x_col, math.cos(angle), math.sin(angle), boxes.data_ptr(), boxes.stride(1), cap,
                 det["scores"].data_ptr(), det["label_preds"].data_ptr(), det["instances"].data_ptr(), det["count"].data_ptr(), sem2box.data_ptr(),
                 float(score_thr), labels.data_ptr(), ins.data_ptr(), hip.stream())

    def _sem2box(self, class_names, semantic2box, ncls, dev):
        """DEVICE int32 table semantic label -> box label (-1: stuff), cached on the head per (class names, device): uploaded once"""
        names = [n for sub in class_names for n in ([sub] if isinstance(sub, str) else sub)]
        things = SEMANTIC2BOX if semantic2box is None else list(semantic2box)
        key = (tuple(names), tuple(things), int(ncls), str(dev))
        cache = self.__dict__.setdefault("_sem2box_cache", {})
        if key not in cache:
            table = [-1] * (ncls + 1)
            for k, name in enumerate(things[:ncls]):
                if name not in names:
                    raise ValueError(f"predict_panoptic: semantic label {k + 1} maps to the box class '{name}', which is not among the head's class_names {names}")
                table[k + 1] = names.index(name)
            cache[key] = torch.tensor(table, dtype=torch.int32, device=dev)
        return cache[key]

    @torch.no_grad()
    def predict_panoptic(self, example, preds_dicts, test_cfg, ret_dict, *, voxel_shape, class_names, sec_id, semantic2box=None, score_thr=0.3,
                         device_only=False):
        """panoptic fusion (seg_head.py:99-168): the per-point semantic labels of ``predict`` plus, for every point, the instance id of
        the nearest box centre of its class, one launch per sample (`pn_panoptic_points_f32`).  Fills ``ret_dict['seg']`` and
        ``ret_dict['ins']`` (lists of {token: (n_i,) int64}; the reference wraps them in iterators) and returns ``ret_dict``.

        ``ret_dict['det']`` holds the per-task lists of ``CenterHead.predict`` under ``test_cfg.panoptic`` (with 'instances'); as in
        the reference only the FIRST task's boxes are used (``ret_dict['det'][0]``, "only works for single group head").  Semantic
        labels 1..len(semantic2box) are thing classes: label k maps to the box class named ``semantic2box[k - 1]``, whose position in
        the flattened ``class_names`` is the box label (ValueError when the name is missing).  Eligible boxes have that label and
        score > ``score_thr``; the point's Cartesian (x, y) -- columns 3:5 of a polar point row (``voxel_shape='cylinder'``), 0:2
        otherwise -- is rotated by the sector angle (``interval * sec_id``; cuboid: ``2 pi / interval * sec_id``) first.  Stuff points
        and things without an eligible box get 0 -- which is also the id of the sweep's first box (the reference's ids start at 0).

        ``device_only=True``: ``ret_dict['det']`` is the device list of ``CenterHead.predict(device_only=True)`` (with 'instances'), all
        samples run in ONE launch (`pn_panoptic_points_batched_f32`: box counts and point offsets are read on the device) and
        ``ret_dict['seg']`` / ``ret_dict['ins']`` are flat (rows,) int64 tensors, one entry per point row of the sector in row order.
        Nothing is read back and, after a first call has cached the class table, nothing is uploaded: the call can be captured."""
        seg = preds_dicts["seg_preds"]
        hip.require_device(seg)
        assert seg.dim() == 4 and seg.stride(1) == 1, "seg_preds must be the channels-last view produced by forward"
        bsz, ncls, h, w = seg.shape
        dev = seg.device
        sem2box = self._sem2box(class_names, semantic2box, ncls, dev)
        sec_id = int(sec_id)
        angle = 0.0
        if sec_id > 0:
            interval = float(test_cfg.get("interval") if hasattr(test_cfg, "get") else getattr(test_cfg, "interval"))
            angle = interval * sec_id if voxel_shape == "cylinder" else 2 * math.pi / interval * sec_id
        x_col = 3 if voxel_shape == "cylinder" else 0
        points = example["points"]
        hip.require_device(points)
        assert points.dim() == 2 and points.dtype == torch.float32 and points.shape[1] >= x_col + 2
        if points.numel() and points.stride(1) != 1:
            points = points.contiguous()
        if device_only:
            det = ret_dict["det"]
            if not (isinstance(det, dict) and "instances" in det and "count" in det):
                raise TypeError("predict_panoptic(device_only=True): ret_dict['det'] must be the device list of CenterHead.predict(device_only=True) under test_cfg.panoptic")
            hip.require_device(*det.values())
            gi, offs = self._flat_rows(example, dev)
            assert gi.shape[0] <= points.shape[0], "valid_grid_ind has more rows than the point list"
            boxes = det["box3d_lidar"]
            cap = int(boxes.shape[1])
            assert boxes.dim() == 3 and boxes.shape[0] == bsz and boxes.dtype == torch.float32 and boxes.stride(2) == 1 and boxes.stride(0) == cap * boxes.stride(1)
            for k, dt in (("scores", torch.float32), ("label_preds", torch.int64), ("instances", torch.int64)):
                assert tuple(det[k].shape) == (bsz, cap) and det[k].dtype == dt and det[k].is_contiguous(), f"the device list's '{k}' must be a contiguous (B, cap) tensor"
            assert tuple(det["count"].shape) == (bsz,) and det["count"].dtype == torch.int32
            labels = torch.empty((gi.shape[0],), dtype=torch.int64, device=dev)
            ins = torch.empty((gi.shape[0],), dtype=torch.int64, device=dev)
            self._launch_batched(seg, gi, offs, labels, points, x_col, angle, det, sem2box, score_thr, ins)
            ret_dict["seg"], ret_dict["ins"] = labels, ins
            return ret_dict
        point_stride = points.stride(0) if points.shape[0] > 1 else points.shape[1]      # (the stride of a 0- or 1-row tensor is arbitrary)
        num = example["num_points"]
        num = [int(v) for v in (num.tolist() if torch.is_tensor(num) else num)]
        assert len(num) == bsz and sum(num) <= points.shape[0], "num_points does not match the batch / the point list"
        dets = ret_dict["det"][0]
        ret_dict["seg"], ret_dict["ins"] = [], []
        start = 0
        for i in range(bsz):
            gi = example["valid_grid_ind"][i]
            gi = (gi if torch.is_tensor(gi) else torch.as_tensor(gi)).to(dev).to(torch.int64).contiguous()
            n = int(gi.shape[0])
            assert gi.dim() == 2 and gi.shape[1] == 3 and n == num[i], "valid_grid_ind[i] must hold one [z, y, x] row per point of sample i"
            det = dets[i]
            boxes, scores = det["box3d_lidar"].float(), det["scores"].float().contiguous()
            box_labels, ids = det["label_preds"].to(torch.int64).contiguous(), det["instances"].to(torch.int64).contiguous()
            hip.require_device(boxes, scores, box_labels, ids)
            if boxes.stride(1) != 1:
                boxes = boxes.contiguous()
            m = int(scores.shape[0])
            assert boxes.shape[0] == m and box_labels.shape[0] == m and ids.shape[0] == m, "the sample's boxes, scores, labels and instances differ in length"
            labels = torch.empty((n,), dtype=torch.int64, device=dev)
            ins = torch.empty((n,), dtype=torch.int64, device=dev)
            base = seg[i].permute(1, 2, 0)                       # (H, W, ncls) view of the (possibly channel-padded) NHWC buffer, read in place
            assert base.stride(2) == 1 and base.stride(0) == w * base.stride(1)
            rows = points[start:start + n]
            hip.call("pn_panoptic_points_f32", base.data_ptr(), h, w, ncls, base.stride(1), gi.data_ptr(), n, rows.data_ptr(), point_stride, x_col,
                     math.cos(angle), math.sin(angle), boxes.data_ptr() if m else None, boxes.stride(0) if m else 2, scores.data_ptr() if m else None,
                     box_labels.data_ptr() if m else None, ids.data_ptr() if m else None, m, sem2box.data_ptr(), float(score_thr), labels.data_ptr(),
                     ins.data_ptr(), hip.stream())
            start += n
            meta = example["metadata"][i]
            token = meta["token"] if isinstance(meta, dict) and "token" in meta else i
            ret_dict["seg"].append({token: labels})
            ret_dict["ins"].append({token: ins})
        return ret_dict
