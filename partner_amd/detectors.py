"""Detectors (orchestration) under the reference's names.

Reference: det3d/models/detectors/single_stage.py:25-50, point_pillars.py:40-110,
voxelnet.py:47-131,171-301.

``PointPillars.forward`` keeps the reference's ``example`` contract.  In eval mode the dynamic
branch runs as one device-side chain with no host synchronisation: linear keys -> bitmap
unique-rank -> bucketing -> fused PFN writing the NHWC canvas -> RPN -> head.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import nn

from . import builder, hip, ops
from .builder import DETECTORS
from .nn_utils import eval_only
from .readers import DynamicPFNet
from .routes import R, S
from .seg_heads import SingleConvHead, device_offsets, host_counts, merge_per_token, prefix_sums, sample_token


@DETECTORS.register_module
class SingleStageDetector(nn.Module):
    def __init__(self, reader, backbone, neck=None, bbox_head=None, seg_head=None, part_head=None, train_cfg=None,
                 test_cfg=None, pretrained=None, nsectors=1):
        super().__init__()
        self.reader = builder.build_reader(reader)
        self.backbone = builder.build_backbone(backbone)
        if neck is not None:
            self.neck = builder.build_neck(neck)
        self.bbox_head = builder.build_bbox_head(bbox_head) if bbox_head is not None else None
        # the `seg` super-task of the nuScenes polar config (SingleConvHead): forward + per-point prediction, eval only
        self.seg_head = builder.build_seg_head(seg_head) if seg_head is not None else None
        if part_head is not None:
            raise NotImplementedError("part heads are outside the hot path (SURVEY.md 2.1); build with part_head=None")
        self.part_head = None
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.init_weights(pretrained)

    @property
    def with_neck(self):
        return hasattr(self, "neck") and self.neck is not None

    def init_weights(self, pretrained=None):
        if pretrained is None:
            return
        sd = torch.load(pretrained, map_location="cpu")
        sd = sd.get("state_dict", sd)
        self.load_state_dict({k[7:] if k.startswith("module.") else k: v for k, v in sd.items()}, strict=False)


def first_stage_device_list(det, example, preds, return_loss, **kwargs):
    """``forward_two_stage``'s tail: decode + NMS of the first stage's head maps into its fixed-capacity device list"""
    if return_loss:
        raise NotImplementedError(f"{type(det).__name__}.forward_two_stage: return_loss=True is not built (the second stage runs inference only)")
    if det.test_cfg is None:
        raise ValueError(f"{type(det).__name__}.forward_two_stage needs the detector's test_cfg (build_detector(cfg, test_cfg=...))")
    return det.bbox_head.predict(example, preds, det.test_cfg, device_only=True, **kwargs)


@DETECTORS.register_module
class PointPillars(SingleStageDetector):
    def __init__(self, reader, backbone, neck, bbox_head, seg_head=None, part_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None):
        super().__init__(reader, backbone, neck, bbox_head, seg_head, part_head, train_cfg, test_cfg, pretrained)

    # -- stage API of the reference (point_pillars.py:40-53) ---------------------------------
    def extract_feat_dynamic(self, data):
        feats, unq = self.reader(data)
        x1 = self.backbone(feats, unq, data["batch_size"], data["grid_size"])
        return x1, self.neck(x1)

    # -- fused device-side chain --------------------------------------------------------------
    def encode_canvas(self, points: torch.Tensor, keys: torch.Tensor, spec: ops.GridSpec, batch: int,
                      n_dev: Optional[torch.Tensor] = None, canvas: Optional[torch.Tensor] = None, return_index=False):
        """points (N,7) + linear voxel keys -> NHWC canvas (B, T, R, C); no host sync.
        ``canvas``: a persistent all-zero map to write into (see ``forward_points``); otherwise a fresh zero-filled one."""
        if not isinstance(self.reader, DynamicPFNet):
            raise NotImplementedError("fused encode path needs a DynamicPFNet reader")
        vi = ops.build_voxel_index(keys, spec, batch, n_dev=n_dev, want_unq=False)
        shape = (batch, spec.grid[1], spec.grid[0], self.reader.out_channels)
        if canvas is None:
            canvas = torch.empty(shape, dtype=torch.float32, device=points.device)
            hip.call("pn_fill_zero", canvas.data_ptr(), canvas.numel() * 4, hip.stream())
        else:
            hip.require_device(canvas)
            assert tuple(canvas.shape) == shape and canvas.is_contiguous() and canvas.dtype == torch.float32
        self.reader.encode(points, vi, None, canvas)
        return (canvas, vi) if return_index else canvas

    def _neck_on_canvas(self, canvas: torch.Tensor, vi) -> torch.Tensor:
        """the backbone on a freshly encoded canvas: plain RPNs take the voxel index with it (sparse first convolution)"""
        from .necks import RPN
        if type(self.neck) is RPN:
            return self.neck.forward_nhwc(canvas, pillars=vi)
        return self.neck.forward_nhwc(canvas)

    def new_canvas(self, batch: int, spec: Optional[ops.GridSpec] = None, device=None) -> torch.Tensor:
        """a zeroed persistent canvas for ``forward_points(..., canvas=)``"""
        spec = spec or ops.GridSpec.from_range(self.reader.pc_range, self.reader.voxel_size)
        device = device or next(self.parameters()).device
        return torch.zeros((batch, spec.grid[1], spec.grid[0], self.reader.out_channels), dtype=torch.float32, device=device)

    def forward_points(self, points: torch.Tensor, sample_offsets: torch.Tensor, batch: int,
                       spec: Optional[ops.GridSpec] = None, canvas: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Hot path from polar-decorated points: grid indices are computed on the device (V1).
        points (N,7) [rho,phi,z,x,y,i,t]; sample_offsets int32 (batch+1).  -> head tensors.
        ``canvas``: a persistent map owned by the caller (``new_canvas``), all zero on entry; the frame's pillars are
        written into it and their cells are cleared again once the backbone has consumed it (a sparse clear of ~28k
        cells instead of a 134 MB fill per frame) -- all zero on exit."""
        eval_only(self, "PointPillars")
        spec = spec or ops.GridSpec.from_range(self.reader.pc_range, self.reader.voxel_size)
        _, keys = ops.grid_index(points, sample_offsets, batch, spec, want_grid_ind=False)
        if canvas is None:
            cv, vi = self.encode_canvas(points, keys, spec, batch, n_dev=sample_offsets[batch:], return_index=True)
            x2 = self._neck_on_canvas(cv, vi)
        else:
            cv, vi = self.encode_canvas(points, keys, spec, batch, n_dev=sample_offsets[batch:], canvas=canvas, return_index=True)
            x2 = self._neck_on_canvas(cv, vi)
            ops.clear_canvas_cells(cv, vi)
        return self.bbox_head(ops.as_nchw(x2))["det_preds"][0]

    def new_index_state(self, batch: int, spec: Optional[ops.GridSpec] = None, device=None):
        """persistent scratch of the fused frame index for ``forward_cart(..., index_state=)``; None when the grid is too large"""
        spec = spec or ops.GridSpec.from_range(self.reader.pc_range, self.reader.voxel_size)
        device = device or next(self.parameters()).device
        return ops.FrameIndexState(spec, batch, device) if ops.FrameIndexState.supported(spec, batch) else None

    def encode_cart(self, cart: torch.Tensor, sample_offsets: torch.Tensor, batch: int, spec: ops.GridSpec,
                    canvas: Optional[torch.Tensor] = None, index_state=None):
        """V0..V5 from Cartesian points: fused frame index (3 launches) + fused PFN writing the canvas cells (1 launch).
        -> (canvas, VoxelIndex, polar points)"""
        if not isinstance(self.reader, DynamicPFNet):
            raise NotImplementedError("fused encode path needs a DynamicPFNet reader")
        shape = (batch, spec.grid[1], spec.grid[0], self.reader.out_channels)
        if index_state is None and not ops.FrameIndexState.supported(spec, batch):
            polar = ops.cart_to_polar(cart)
            _, keys = ops.grid_index(polar, sample_offsets, batch, spec, want_grid_ind=False)
            cv, vi = self.encode_canvas(polar, keys, spec, batch, n_dev=sample_offsets[batch:], canvas=canvas, return_index=True)
            return cv, vi, polar
        polar, vi = ops.fused_voxel_index(cart, sample_offsets, batch, spec, index_state)
        if canvas is None:
            canvas = torch.empty(shape, dtype=torch.float32, device=cart.device)
            hip.call("pn_fill_zero", canvas.data_ptr(), canvas.numel() * 4, hip.stream())
        else:
            hip.require_device(canvas)
            assert tuple(canvas.shape) == shape and canvas.is_contiguous() and canvas.dtype == torch.float32
        vi.index_cleared = self.reader.encode(polar, vi, None, canvas, clear_index=index_state)      # (r6: the reader's launch zeroes the index counters)
        return canvas, vi, polar

    def forward_sweeps(self, raw: torch.Tensor, sweep_offsets: torch.Tensor, transforms: torch.Tensor, time_lags: torch.Tensor, spec: ops.GridSpec,
                       canvas: torch.Tensor, index_state, canvas_may_stay_dirty: bool = False, min_distance: float = 1.0) -> Dict[str, torch.Tensor]:
        """``forward_cart`` for ONE multi-sweep frame handed over as its raw sweeps (BASELINE configs[4]): the accumulation
        (``ops.accumulate_sweeps``: remove_close, rigid transforms, time lags) happens inside the frame index's first launch
        (``ops.fused_voxel_index_sweeps``, r6) -- no compaction, no Cartesian copy, three launches less.  Same head tensors, bit for bit
        (the reader's sums and maxima do not depend on the order or the numbering of a pillar's points)."""
        eval_only(self, "PointPillars")
        if not isinstance(self.reader, DynamicPFNet):
            raise NotImplementedError("fused encode path needs a DynamicPFNet reader")
        hip.require_device(canvas)
        assert tuple(canvas.shape) == (1, spec.grid[1], spec.grid[0], self.reader.out_channels) and canvas.is_contiguous()
        polar, vi = ops.fused_voxel_index_sweeps(raw, sweep_offsets, transforms, time_lags, spec, index_state, min_distance)
        cleared = self.reader.encode(polar, vi, None, canvas, clear_index=index_state)
        x2 = self._neck_on_canvas(canvas, vi)
        leave = canvas_may_stay_dirty and self.seg_head is None and getattr(self.neck, "canvas_read_by_pillars_only", False)
        ops.clear_frame_cells(None if leave else canvas, vi, None if cleared else index_state)
        return self.bbox_head(ops.as_nchw(x2))["det_preds"][0]

    def scatter_stage(self, cart: torch.Tensor, sample_offsets: torch.Tensor, batch: int, spec: ops.GridSpec, canvas: torch.Tensor,
                      index_state=None):
        """V0..V5 alone, exactly as a frame of ``forward_cart(canvas=, index_state=)`` runs them (fused frame index, fused PFN
        writing the persistent canvas, sparse clear): what bench.py's ``roofline_scatter`` times.
        -> the VoxelIndex (voxel count on the device)"""
        cv, vi, _ = self.encode_cart(cart, sample_offsets, batch, spec, canvas=canvas, index_state=index_state)
        ops.clear_frame_cells(cv, vi, getattr(vi, "state", None) if (index_state is not None and not getattr(vi, "index_cleared", False)) else None)
        return vi

    def forward_cart(self, cart: torch.Tensor, sample_offsets: torch.Tensor, batch: int, spec: Optional[ops.GridSpec] = None,
                     canvas: Optional[torch.Tensor] = None, index_state=None, canvas_may_stay_dirty: bool = False) -> Dict[str, torch.Tensor]:
        """The hot path from CARTESIAN points (N, 5) [x, y, z, intensity, dt] resident on the device: V0 .. H2, head tensors out.
        ``canvas`` / ``index_state``: persistent buffers owned by the caller (``new_canvas`` / ``new_index_state``), all zero on
        entry and on exit (the frame's cells are cleared once the backbone's first layer has consumed the canvas).
        ``canvas_may_stay_dirty`` (r6; the frame engines, whose canvas nobody else sees): where the first convolution took the row-band pillar
        form -- it reads exactly the cells of the frame's key list and nothing else does -- the old frame's feature rows are left in the
        canvas (only the index counters are cleared): 14.5 MB of zero stores less per 30k-point frame, 92 MB per 300k-point frame.  Such a
        canvas must never reach a dense consumer."""
        eval_only(self, "PointPillars")
        spec = spec or ops.GridSpec.from_range(self.reader.pc_range, self.reader.voxel_size)
        cv, vi, _ = self.encode_cart(cart, sample_offsets, batch, spec, canvas=canvas, index_state=index_state)
        x2 = self._neck_on_canvas(cv, vi)
        if canvas is not None or index_state is not None:
            leave = (canvas_may_stay_dirty and canvas is not None and index_state is not None and self.seg_head is None
                     and getattr(self.neck, "canvas_read_by_pillars_only", False))
            ops.clear_frame_cells(None if leave else (cv if canvas is not None else None), vi, None if getattr(vi, "index_cleared", False) else index_state)
        return self.bbox_head(ops.as_nchw(x2))["det_preds"][0]

    def extract_preds(self, example) -> Dict[str, object]:
        """reference ``example`` dict (dynamic branch keys) -> {'det_preds': [...]}"""
        return self._heads(*self._neck_maps(example))

    def _neck_maps(self, example):
        """reference ``example`` dict -> (the NHWC canvas, the NHWC neck output)"""
        eval_only(self, "PointPillars")
        if "voxels" in example:   # hard-voxel (static) branch, point_pillars.py:27-38 / 60-76
            voxels, coords = example["voxels"], example["coordinates"]
            hip.require_device(voxels, coords)
            feats = self.reader(voxels, example["num_points"], coords)
            x1 = self.backbone(feats, coords, len(example["num_voxels"]), [int(v) for v in example["shape"][0]])
            x1h = ops.to_nhwc(x1)
            x2 = self.neck.forward_nhwc(x1h) if self.with_neck else x1h
            return x1h, x2
        points, grid_ind = example["points"], example["grid_ind"]
        hip.require_device(points, grid_ind)
        batch = len(example["num_points"])
        g = [int(v) for v in example["grid_size"][0]]
        spec = ops.GridSpec.from_range(self.reader.pc_range, self.reader.voxel_size)
        if list(spec.grid) != g:
            raise ValueError(f"example grid_size {g} does not match the reader's voxel grid {list(spec.grid)}")
        keys = ops.keys_from_grid_ind(grid_ind.to(torch.int64).contiguous(), spec, batch)
        canvas, vi = self.encode_canvas(points.contiguous(), keys, spec, batch, return_index=True)
        x2 = self._neck_on_canvas(canvas, vi)
        return canvas, x2

    def forward_two_stage(self, example, return_loss=False, **kwargs):
        """the first stage of a TwoStageDetector (point_pillars.py:112-140, two_stage.py:155-166), inference: whatever ``extract_preds``
        accepts -> (the device list of ``bbox_head.predict(device_only=True)``, the NHWC neck output); nothing is read back"""
        preds, x2 = self.two_stage_preds(example)
        return first_stage_device_list(self, example, preds, return_loss, **kwargs), x2

    def two_stage_preds(self, example):
        """-> (the head's prediction dict, the NHWC neck output): what ``forward_two_stage`` decodes, and what ``TwoStageTrainStep`` takes the
        first stage's loss from"""
        x1h, x2 = self._neck_maps(example)
        return self._heads(x1h, x2), x2

    def _heads(self, x1_nhwc: torch.Tensor, x2_nhwc: torch.Tensor) -> Dict[str, object]:
        """point_pillars.py:91-96: the detection head on the RPN output, the segmentation head (when the config has one) on the
        canvas + the RPN output"""
        preds = {}
        if self.bbox_head is not None:
            preds.update(self.bbox_head(ops.as_nchw(x2_nhwc)))
        if self.seg_head is not None:
            seg = self.seg_head.forward_nhwc(x1_nhwc, x2_nhwc)
            preds["seg_preds"] = seg.permute(0, 3, 1, 2)[:, :self.seg_head.num_classes]
        return preds

    def forward(self, example, return_loss=True, **kwargs):
        preds = self.extract_preds(example)
        if return_loss:
            losses = self.bbox_head.loss(example, preds)
            if self.seg_head is not None:      # point_pillars.py:99-103: both super-tasks' terms in one dict
                losses.update(self.seg_head.loss(example, preds))
            return losses
        if kwargs.get("raw_preds", False) or self.test_cfg is None:
            return preds
        ret = {}
        if self.bbox_head is not None:
            ret["det"] = self.bbox_head.predict(example, preds, self.test_cfg, **kwargs)
        if self.seg_head is not None:
            ret["seg"] = self.seg_head.predict(example, preds, self.test_cfg)
        return ret


@DETECTORS.register_module
class PolarStream(PointPillars):
    """PolarStream (det3d/models/detectors/polarstream.py:7-180): a sweep given as a LIST of azimuth-sector examples is processed
    sector by sector, the neck (RPNTECP / RPNBDCP) pads every sector with the context rows the previous sector left behind, and the
    per-sector detections are rotated back into the sweep's frame and concatenated (single_stage.py:83-165).  A single example (dict)
    is the full-sweep case.  Eval mode; stateful NMS across sectors (test_cfg.stateful_nms, the default of the reference's 4-sector
    configs) is supported.  With a segmentation head every sector also yields per-point semantic labels ('seg'), and with
    test_cfg.panoptic per-point instance ids ('ins', polarstream.py:161-171): the boxes' ids are carried from sector to sector like
    the stateful NMS's detections, and the merged detections keep their 'instances' (the reference drops them) so that 'ins' can be
    mapped back to a box.  Sector examples that carry ``key_points_index`` (per sample, the positions of the sector's points in the
    dataset's point list) get 'seg' / 'ins' back in that order (merge_sectors, single_stage.py:97-128)."""

    def forward_one_sector(self, example, return_loss=True, **kwargs):
        eval_only(self, "PolarStream")
        points, grid_ind = example["points"], example["grid_ind"]
        hip.require_device(points, grid_ind)
        batch = len(example["num_points"])
        g = [int(v) for v in example["grid_size"][0]]
        # the sector grid: the reader's range with the azimuth axis cut to the sector (voxelization.py:318-323)
        spec = ops.GridSpec(tuple(float(v) for v in self.reader.pc_range[:3]), tuple(float(v) for v in self.reader.voxel_size), (g[0], g[1], g[2]))
        keys = ops.keys_from_grid_ind(grid_ind.to(torch.int64).contiguous(), spec, batch)
        canvas = self.encode_canvas(points.contiguous(), keys, spec, batch)
        nxt = []
        if hasattr(self.neck, "_pad_feature_only") or not hasattr(self.neck, "forward_nhwc"):
            raise NotImplementedError("PolarStream drives the trailing-edge neck (RPNTECP) or the plain RPN; RPNBDCP is driven by PolarStreamBDCP's two-sweep loop")
        from .necks_context import RPNTECP
        if isinstance(self.neck, RPNTECP):      # the trailing-edge neck takes (and returns) the context rows
            x2, nxt = self.neck.forward_nhwc(canvas, kwargs.get("prev_context", []), kwargs.get("sec_id", 0))
        else:                                   # plain RPN: no context, its own signature (return_blocks, pillars)
            x2 = self.neck.forward_nhwc(canvas)
        if return_loss:
            preds = self.bbox_head(ops.as_nchw(x2))
        else:                                   # polarstream.py:149-152: the seg head (when there is one) on the sector canvas + the neck output
            preds = self._heads(canvas, x2)
        ret = {}
        if return_loss:
            ret.update(self.bbox_head.loss(example, preds))
        elif kwargs.get("raw_preds", False) or self.test_cfg is None:
            ret.update(preds)
        else:
            sec_id = kwargs.get("sec_id", 0)
            dev_only = bool(kwargs.get("device_only", False))      # device lists / flat per-point outputs: no readback (``forward``)
            ret["det"] = self.bbox_head.predict(example, preds, self.test_cfg, sec_id=sec_id, prev_dets=kwargs.get("prev_dets"), device_only=dev_only)
            if self.seg_head is not None:      # polarstream.py:163-171
                if self._test_flag("panoptic"):
                    self.seg_head.predict_panoptic(example, preds, self.test_cfg, ret, voxel_shape=self.bbox_head.voxel_shape,
                                                   class_names=self.bbox_head.class_names, sec_id=sec_id, device_only=dev_only)
                else:
                    ret["seg"] = self.seg_head.predict(example, preds, self.test_cfg, device_only=dev_only)
        if len(nxt):
            ret["next_context"] = nxt
        return ret

    def forward(self, example, return_loss=True, **kwargs):
        """``device_only=True`` (inference): the sectors' detection lists stay on the device (``CenterHead.predict(device_only=True)``)
        and the per-point outputs are flat tensors, so that from the first launch to the last nothing is read back or synchronised and
        the sweep can be captured in one graph.  Returns 'det': the LAST sector's device list when the list is carried from sector to
        sector (stateful NMS / panoptic), otherwise the list of per-sector device lists; 'seg' (and 'ins' under panoptic): lists of
        per-sector flat (rows,) int64 tensors.  ``sweep_to_host`` turns that into what this method returns without the flag."""
        if isinstance(example, dict):
            return self.forward_one_sector(example, return_loss, **kwargs)
        stateful, panoptic = self._test_flag("stateful_nms"), self._test_flag("panoptic")
        dev_only = bool(kwargs.get("device_only", False)) and not return_loss and not kwargs.get("raw_preds", False) and self.test_cfg is not None
        rets, prev = [], []
        for i, ex in enumerate(example):
            kw = dict(kwargs, prev_context=prev, sec_id=i)
            if (stateful or panoptic) and i > 0 and "det" in rets[-1]:
                kw["prev_dets"] = rets[-1]["det"]     # polarstream.py:91-92
            r = self.forward_one_sector(ex, return_loss, **kw)
            prev = r.pop("next_context", []) if i < len(example) - 1 else []
            r.pop("next_context", None)
            if "key_points_index" in ex and not dev_only:      # polarstream.py:99-100; the device form leaves the order to sweep_to_host
                r["key_points_index"] = ex["key_points_index"]
            rets.append(r)
        if dev_only:
            out = {"det": rets[-1]["det"] if (stateful or panoptic) else [r["det"] for r in rets]}
            for k in ("seg", "ins"):
                if k in rets[0]:
                    out[k] = [r[k] for r in rets]
            return out
        out = self.merge_sectors(rets, len(example[-1]["num_points"]), stateful or panoptic)
        if (stateful or panoptic) and "det" in out:
            for det, meta in zip(out["det"], example[-1].get("metadata", [None] * len(out["det"]))):
                det["metadata"] = meta
        return out

    @staticmethod
    def sweep_to_host(out, examples):
        """The result of ``forward(examples, return_loss=False, device_only=True)`` -> exactly what ``forward(examples,
        return_loss=False)`` returns: per-sample detections cut to their counts with 'metadata' (a carried list: the last sector's,
        with 'instances' under panoptic; otherwise the sectors' lists concatenated, with 'cells'), and per-sample {token: tensor} dicts
        for 'seg' / 'ins', the sectors' rows of a sample concatenated in sector order.  ONE readback, of the counts; the per-point
        outputs are split by the host ``num_points``.  Sector examples that all carry ``key_points_index`` put 'seg' / 'ins' into dataset
        order, as ``merge_sectors`` does, indexing on the tensors' device.  Index bookkeeping only: runs on whatever device the tensors live on."""
        res = {}
        det = out.get("det")
        fields = ("box3d_lidar", "scores", "label_preds")
        if isinstance(det, dict):        # carried from sector to sector: the last sector's list is the sweep's
            counts = det["count"].tolist()
            metas = examples[-1].get("metadata", [None] * len(counts))
            res["det"] = []
            for i, n in enumerate(counts):
                d = {k: det[k][i, :n] for k in fields + (("instances",) if "instances" in det else ())}
                d["metadata"] = metas[i]
                res["det"].append(d)
        elif det is not None:            # one list per sector: concatenated per sample (single_stage.py:118-135)
            counts = torch.stack([d["count"] for d in det]).tolist()
            metas = examples[0].get("metadata", [None] * len(counts[0]))
            res["det"] = []
            for i in range(len(counts[0])):
                d = {k: torch.cat([s[k][i, :counts[j][i]] for j, s in enumerate(det)]) for k in fields + ("cells",)}
                d["metadata"] = metas[i]
                res["det"].append(d)
        for key in ("seg", "ins"):
            if key not in out:
                continue
            sectors = []
            for ex, flat in zip(examples, out[key]):      # a sector's flat rows cut into its samples' by the host counts
                acc = prefix_sums(host_counts(ex["num_points"]))
                sectors.append([{sample_token(ex["metadata"], i): flat[lo:hi]} for i, (lo, hi) in enumerate(zip(acc[:-1], acc[1:]))])
            res[key] = merge_per_token(sectors, len(examples[0]["num_points"]))
        if ("seg" in res or "ins" in res) and all("key_points_index" in ex for ex in examples):
            batch = len(examples[0]["num_points"])
            index = [PolarStream._cat_index([ex["key_points_index"][i] for ex in examples]) for i in range(batch)]
            for key in ("seg", "ins"):
                if key in res:
                    res[key] = PolarStream._to_dataset_order(res[key], index)
            res["key_points_index"] = index      # merge_sectors returns it too (single_stage.py:97-104)
        return res

    @staticmethod
    def _cat_index(parts):
        """one sample's ``key_points_index`` pieces (numpy arrays, lists or tensors), sector by sector -> one int64 tensor, on the device
        the pieces live on (nothing is read back)"""
        return torch.cat([torch.as_tensor(p).reshape(-1).to(torch.int64) for p in parts])

    @staticmethod
    def _to_dataset_order(per_sample, index):
        """single_stage.py:118-128: per sample and token, ``out = zeros_like(v); out[index] = v`` -- the sectors' rows back at their
        positions in the dataset's point list; positions no row names read 0"""
        out = []
        for m, idx in zip(per_sample, index):
            d = {}
            for token, v in m.items():
                tmp = v.new_zeros(v.shape)
                tmp[idx.to(v.device)] = v
                d[token] = tmp
            out.append(d)
        return out

    def _test_flag(self, name) -> bool:
        cfg = self.test_cfg
        if cfg is None:
            return False
        return bool(cfg.get(name, False) if hasattr(cfg, "get") else getattr(cfg, name, False))

    def merge_sectors(self, sectors, batch_size, stateful=False):
        """single_stage.py:83-165 for the keys this build produces: losses are lists concatenated over sectors, detections are
        concatenated per sample; with stateful NMS or panoptic fusion (``stateful``) the LAST sector's per-task lists already hold the
        whole sweep (merge_dets :137-153: tasks concatenated, labels offset by the preceding tasks' class counts; 'instances', where the
        lists carry them, are kept); 'seg' / 'ins' are concatenated per sample and token in sector order (:106-116); 'key_points_index'
        (per sector a list of one index array per sample) is concatenated per sample (:97-104), and 'seg' / 'ins' are then scattered to
        those positions (:118-128)"""
        out = {}
        for k in sectors[0]:
            vals = [s[k] for s in sectors]
            if "loss" in k:
                out[k] = [v for lst in vals for v in lst]
            elif k == "det" and stateful:
                tasks = vals[-1]
                merged = []
                for i in range(len(tasks[0])):
                    flag, labels = 0, []
                    for j, ncls in enumerate(self.bbox_head.num_classes[:len(tasks)]):
                        labels.append(tasks[j][i]["label_preds"] + flag)
                        flag += ncls
                    merged.append(dict(box3d_lidar=torch.cat([t[i]["box3d_lidar"] for t in tasks]), scores=torch.cat([t[i]["scores"] for t in tasks]),
                                       label_preds=torch.cat(labels)))
                    if all("instances" in t[i] for t in tasks):
                        merged[-1]["instances"] = torch.cat([t[i]["instances"] for t in tasks])
                out[k] = merged
            elif k == "det":
                merged = []
                for i in range(len(vals[0])):
                    d = {}
                    for f in vals[0][0]:
                        d[f] = vals[0][i][f] if f == "metadata" else torch.cat([v[i][f] for v in vals])
                    merged.append(d)
                out[k] = merged
            elif k in ("det_preds", "seg_preds"):
                out[k] = vals
            elif k in ("seg", "ins"):
                out[k] = merge_per_token(vals, batch_size)
            elif k == "key_points_index":
                out[k] = [PolarStream._cat_index([sec[i] for sec in vals]) for i in range(batch_size)]
        if "key_points_index" in out:
            for k in ("seg", "ins"):
                if k in out:
                    out[k] = PolarStream._to_dataset_order(out[k], out["key_points_index"])
        return out


@DETECTORS.register_module
class PolarStreamBDCP(PolarStream):
    """PolarStream with bidirectional context padding (det3d/models/detectors/polarstream.py:180-470): ``forward`` takes TWO sweeps.
    The previous sweep runs in ``feature_only`` mode (all its sectors stacked in the batch axis, sector-major); the per-layer inputs
    of the neck (RPNBDCP) are glued back into whole-sweep maps and warped into the current sweep's frame by the ego rotation
    (``transform_matrix`` (bs, 2, 2); `pn_polar_warp_f32`).  The current sweep is then streamed sector by sector: trailing-edge context
    from the sector before, leading-edge context from the warped previous sweep.  Eval mode; the detection super-task and, with a seg
    head, per-point labels ('seg') and under test_cfg.panoptic per-point instance ids ('ins', polarstream.py:423-460): the detection list
    is then carried from sector to sector as under stateful NMS and keeps its 'instances'.  All sectors' logits exist before the first
    NMS, so the device path runs the whole sweep's per-point work as ONE launch after the last NMS (`pn_panoptic_points_sweep_f32`).
    With more than one sector an example's ``key_points_index`` (per stacked sample, the positions of its points in the dataset's point
    list) puts 'seg' / 'ins' into dataset order (polarstream.py:453-454, single_stage.py:97-128); with one sector it is not read, as in
    the reference.  ``valid_grid_ind`` must hold one row per point of the stacked point list."""

    def __init__(self, reader, backbone, neck, bbox_head, seg_head=None, part_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 nsectors=1):
        neck = dict(neck)
        neck["nsectors"] = nsectors          # polarstream.py:205
        super().__init__(reader, backbone, neck, bbox_head, seg_head, part_head, train_cfg, test_cfg, pretrained)
        self.nsectors = int(nsectors)

    def _canvas(self, example):
        points, grid_ind = example["points"], example["grid_ind"]
        hip.require_device(points, grid_ind)
        batch = len(example["num_points"])
        g = [int(v) for v in example["grid_size"][0]]
        spec = ops.GridSpec(tuple(float(v) for v in self.reader.pc_range[:3]), tuple(float(v) for v in self.reader.voxel_size), (g[0], g[1], g[2]))
        keys = ops.keys_from_grid_ind(grid_ind.to(torch.int64).contiguous(), spec, batch)
        return self.encode_canvas(points.contiguous(), keys, spec, batch), batch

    def _get(self, k, d=None):
        return self.test_cfg.get(k, d) if hasattr(self.test_cfg, "get") else getattr(self.test_cfg, k, d)

    def warp_prev_sweep(self, cur_sweep, transform, bs):
        """per-layer inputs of the stacked sectors (nsectors * bs, h, w, c) -> whole-sweep maps (bs, nsectors * h, w, c) warped by the
        (bs, 2, 2) rotation (polarstream.py:340-358)"""
        pr = self._get("pc_range")
        rot = transform.to(cur_sweep[0].device).float().contiguous()
        out = []
        for x in cur_sweep:
            n, h, w, c = x.shape
            assert n == self.nsectors * bs and x.is_contiguous()
            warped = torch.empty((bs, self.nsectors * h, w, c), dtype=torch.float32, device=x.device)
            hip.call("pn_polar_warp_f32", x.data_ptr(), rot.data_ptr(), bs, self.nsectors, self.nsectors * h, w, c, float(pr[0]), float(pr[3]), float(pr[1]),
                     float(pr[4]), warped.data_ptr(), hip.stream())
            out.append(warped)
        return out

    def warp_prev_strips(self, cur_sweep, transform, bs):
        """``warp_prev_sweep`` for the rows the streaming pass reads and nothing else: ONE `pn_polar_warp_strips_f32` launch for all layers
        -> per layer a ``PrevStrips`` pack (bs, (nsectors + 1) * pad, w, c), bit for bit the rows of the whole warped map.  ``transform``
        may live on the device already (nothing is uploaded then)."""
        from .necks_context import PrevStrips
        pr = self._get("pc_range")
        nsec = self.nsectors
        dev = cur_sweep[0].device
        rot = torch.as_tensor(transform)[:bs].to(dev).float().contiguous()
        pad = max(int(cc.padding) for blk in self.neck.blocks for cc in blk._modules.values())
        rows = (nsec + 1) * pad
        sizes = [bs * rows * x.shape[2] * x.shape[3] for x in cur_sweep]
        flat = torch.empty((sum(sizes),), dtype=torch.float32, device=dev)
        jobs = (hip.WarpStripJob * len(cur_sweep))()
        out, at = [], 0
        for k, x in enumerate(cur_sweep):
            n, hs, w, c = x.shape
            assert n == nsec * bs and x.is_contiguous() and x.dtype == torch.float32
            strips = flat[at:at + sizes[k]].view(bs, rows, w, c)
            at += sizes[k]
            jobs[k].in_, jobs[k].out, jobs[k].h, jobs[k].w, jobs[k].c = x.data_ptr(), strips.data_ptr(), nsec * hs, w, c
            out.append(PrevStrips(strips, nsec, pad, hs))
        hip.call("pn_polar_warp_strips_f32", jobs, len(cur_sweep), rot.data_ptr(), bs, nsec, pad, float(pr[0]), float(pr[3]), float(pr[1]), float(pr[4]),
                 hip.stream())
        return out

    def _stream_sectors(self, canvas, prev_sweep, bs, mode):
        """the current sweep through the neck, sector by sector (polarstream.py:386-402) -> the stacked neck output"""
        nsec = self.nsectors
        if nsec == 1:
            return self.neck.forward_nhwc(canvas, prev_sweep=prev_sweep, nsectors=1, mode=mode)[0]
        outs, ctx = [], []
        for j in range(nsec):
            y, ctx = self.neck.forward_nhwc(canvas[j * bs:(j + 1) * bs].contiguous(), prev_sweep=prev_sweep, prev_context=ctx, sec_id=j, nsectors=nsec,
                                            mode=mode)
            outs.append(y)
        return torch.cat(outs, 0)

    def _refuse_unbuilt(self, return_loss):
        """``forward`` runs the folded eval-mode kernels; with ``return_loss`` it returns the loss of those predictions.  Training -- batch
        statistics and gradients -- is ``train_stream.PolarStreamBDCPTrainStep``."""
        eval_only(self, "PolarStreamBDCP")
        if not return_loss and self._test_flag("panoptic") and self.seg_head is None:
            raise NotImplementedError("PolarStreamBDCP: test_cfg.panoptic (polarstream.py:423-460) needs a seg head -- the panoptic fusion assigns the "
                                      "boxes' instance ids to the seg head's per-point labels")

    def _sector(self, preds, example, i, bs, per_point=False):
        """sector i's slice of the stacked predictions and of the stacked example: 'metadata', 'pc_range' (when the example has one) and,
        ``per_point``, 'num_points' / 'valid_grid_ind' -> (preds, example)"""
        cut = slice(i * bs, (i + 1) * bs)
        pr = {"det_preds": [{k: v[cut] for k, v in t.items()} for t in preds["det_preds"]]}
        if "seg_preds" in preds:
            pr["seg_preds"] = preds["seg_preds"][cut]
        ex = dict(metadata=example.get("metadata", [None] * (self.nsectors * bs))[cut])
        if "pc_range" in example:
            ex["pc_range"] = example["pc_range"][cut]
        if per_point:
            ex.update({k: example[k][cut] for k in ("num_points", "valid_grid_ind")})
        return pr, ex

    def forward_one_sweep(self, example, mode="feature_only", return_loss=False, **kwargs):
        self._refuse_unbuilt(return_loss)
        canvas, batch = self._canvas(example)
        nsec = self.nsectors
        bs = batch // nsec
        if mode == "feature_only":
            _, cur = self.neck.forward_nhwc(canvas, nsectors=nsec, mode="feature_only")
            return self.warp_prev_sweep(cur, torch.as_tensor(example["transform_matrix"])[:bs], bs)
        x2 = self._stream_sectors(canvas, kwargs["prev_sweep"], bs, mode)
        preds = self._heads(canvas, x2)             # polarstream.py:404-408: the seg head (when there is one) on the stacked canvases + neck output
        if return_loss:                             # polarstream.py:409-416: both super-tasks' terms on the STACKED predictions, one dict
            losses = self.bbox_head.loss(example, preds)
            if self.seg_head is not None:
                losses.update(self.seg_head.loss(example, preds))
            return losses
        if kwargs.get("raw_preds", False) or self.test_cfg is None:
            return [self._sector(preds, example, i, bs)[0] for i in range(nsec)]
        stateful, panoptic = bool(self._get("stateful_nms", False)), self._test_flag("panoptic")
        rets, prev_dets = [], None
        key_index = self._key_index_lists(example) if (self.seg_head is not None and nsec > 1) else None
        cum = 0
        for i in range(nsec):
            pr, ex = self._sector(preds, example, i, bs, per_point=self.seg_head is not None)
            det = self.bbox_head.predict(ex, pr, self.test_cfg, sec_id=i, prev_dets=prev_dets)
            rets.append({"det": det})
            prev_dets = det if (stateful or panoptic) and i < nsec - 1 else None      # polarstream.py:444-448
            if self.seg_head is not None:           # polarstream.py:449-463
                if key_index is not None:           # :453-454 (one sector: not read)
                    rets[i]["key_points_index"] = key_index[i * bs:(i + 1) * bs]
                if panoptic:                        # :455-460: the sector's slice of the stacked point list, one row per valid_grid_ind row
                    n = sum(host_counts(ex["num_points"]))
                    ex["points"] = example["points"][cum:cum + n]
                    cum += n
                    self.seg_head.predict_panoptic(ex, pr, self.test_cfg, rets[i], voxel_shape=self.bbox_head.voxel_shape,
                                                   class_names=self.bbox_head.class_names, sec_id=i)
                else:
                    rets[i]["seg"] = self.seg_head.predict(ex, pr, self.test_cfg)
        return rets

    def _key_index_lists(self, example):
        """``example['key_points_index']`` as the reference has it, one index array per stacked sample (None without the key); a flat
        tensor in stacked row order -- the device path's form -- is cut by the host ``num_points``"""
        kpi = example.get("key_points_index")
        if kpi is None or not torch.is_tensor(kpi):
            return kpi
        return list(torch.split(kpi.reshape(-1), host_counts(example["num_points"])))

    def _key_index_flat(self, example, rows, dev):
        """the device path's form of ``example['key_points_index']``: ONE (rows,) int64 device tensor in stacked row order.  A device tensor
        is taken as it is; the reference's per-sample list is concatenated and uploaded once and kept in the example (not capturable)."""
        kpi = example["key_points_index"]
        if not (torch.is_tensor(kpi) and kpi.is_cuda):
            flat = example.get("key_points_index_flat")
            if flat is None:
                parts = [kpi] if torch.is_tensor(kpi) else list(kpi)
                flat = example["key_points_index_flat"] = self._cat_index(parts).to(dev)
            kpi = flat
        kpi = kpi.reshape(-1).to(torch.int64).contiguous()
        assert kpi.shape[0] == rows, "key_points_index must hold one entry per point row"
        return kpi

    def _sample_offsets(self, example, dev):
        """(bs + 1,) int32 device offsets of the samples' points in dataset order (a sample's points of all sectors together) and their
        host values: ``example['sample_offsets']`` when present, otherwise built once from the host ``num_points`` and kept there"""
        num = host_counts(example["num_points"])
        bs = len(num) // self.nsectors
        acc = prefix_sums(sum(num[b::bs]) for b in range(bs))
        offs = device_offsets(example, "sample_offsets", acc, dev)
        assert offs.dtype == torch.int32 and offs.dim() == 1 and offs.is_contiguous() and offs.shape[0] == bs + 1, \
            "sample_offsets must be a contiguous int32 (bs + 1,) tensor"
        return offs, acc

    def prev_sweep_strips(self, example):
        """the previous sweep's pass of the device path: canvas, the neck up to its last layer's input, one strip-warp launch
        -> per layer a ``PrevStrips`` pack (what ``forward_one_sweep(example, 'feature_only')`` returns as whole maps)"""
        canvas, batch = self._canvas(example)
        _, cur = self.neck.forward_nhwc(canvas, nsectors=self.nsectors, mode="feature_only", inputs_only=True)
        return self.warp_prev_strips(cur, example["transform_matrix"], batch // self.nsectors)

    def _forward_device(self, example, **kwargs):
        """``forward(..., device_only=True)``: the two-sweep step with nothing read back or synchronised, so that it can be captured in one
        graph.  The previous sweep runs the canvas and the neck up to its last layer's input (no last convolution, no deblocks: nobody
        reads them), and ONE launch warps the border rows the current sweep's streaming pass reads; with one sector the padding is
        circular and the previous sweep is skipped altogether.  The current sweep is the host path's, with the heads' ``device_only`` calls
        per sector.  Under test_cfg.panoptic the list is carried from sector to sector (fresh fixed-capacity buffers of
        ``nms_post_max_size * (sector + 1)`` rows each), and after the last NMS ONE launch writes every sector's labels and instance ids
        (``SingleConvHead.predict_panoptic_sweep``); with ``key_points_index`` (more than one sector) that launch -- the labels alone
        without panoptic -- writes them in dataset order.  ``valid_grid_ind`` must hold one row per point of ``points``."""
        self._refuse_unbuilt(False)
        prev_ex, ex = example
        nsec = self.nsectors
        prev_sweep = self.prev_sweep_strips(prev_ex) if nsec > 1 else []
        canvas, batch = self._canvas(ex)
        bs = batch // nsec
        preds = self._heads(canvas, self._stream_sectors(canvas, prev_sweep, bs, "eval"))
        stateful, panoptic = bool(self._get("stateful_nms", False)), self._test_flag("panoptic")
        carry = stateful or panoptic
        dets, segs, prev_dets = [], [], None
        ordered = self.seg_head is not None and nsec > 1 and ex.get("key_points_index") is not None
        sweep_launch = panoptic or ordered      # the per-point work of all sectors in one launch after the loop
        if self.seg_head is not None:
            gi, offs = SingleConvHead._flat_rows(ex, canvas.device, stacked=True)
            first = prefix_sums(host_counts(ex["num_points"]))
            if sweep_launch:
                assert gi.dim() == 2 and gi.shape[1] == 3 and gi.shape[0] == first[-1] <= ex["points"].shape[0], \
                    "valid_grid_ind must hold one [z, y, x] row per point of the stacked point list"
        for i in range(nsec):
            pr, sec = self._sector(preds, ex, i, bs)
            prev_dets = self.bbox_head.predict(sec, pr, self.test_cfg, sec_id=i, prev_dets=prev_dets if carry else None, device_only=True)
            dets.append(prev_dets)
            if self.seg_head is not None and not sweep_launch:
                # the sector's samples are rows [offs[i * bs], offs[(i + 1) * bs]) of the sweep's flat list: the kernel takes absolute offsets, so
                # the head gets the whole list with the sector's offsets and writes the sector's rows, which the host counts cut out
                rows = dict(valid_grid_ind=gi, point_offsets=offs[i * bs:(i + 1) * bs + 1])
                labels = self.seg_head.predict(rows, pr, self.test_cfg, device_only=True)
                segs.append(labels[first[i * bs]:first[(i + 1) * bs]])
        out = {"det": dets[-1] if carry else dets}
        if sweep_launch:
            kw = {}
            if ordered:
                sample_offs, acc = self._sample_offsets(ex, canvas.device)
                kw = dict(key_points_index=self._key_index_flat(ex, gi.shape[0], canvas.device), out_offsets=sample_offs, out_total=acc[-1])
            labels, ins = self.seg_head.predict_panoptic_sweep(preds["seg_preds"], gi, offs, ex["points"], dets if panoptic else None, self.test_cfg,
                                                               voxel_shape=self.bbox_head.voxel_shape, class_names=self.bbox_head.class_names,
                                                               nsectors=nsec, **kw)
            cuts = acc if ordered else [first[i * bs] for i in range(nsec + 1)]      # per sample in dataset order / per sector in stacked order
            out["seg"] = [labels[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
            if panoptic:
                out["ins"] = [ins[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
            if ordered:
                out["dataset_order"] = True
        elif self.seg_head is not None:
            out["seg"] = segs
        return out

    def sweep_to_host(self, out, cur_example):
        """The result of ``forward([prev, cur], return_loss=False, device_only=True)`` -> exactly what ``forward([prev, cur],
        return_loss=False)`` returns, with ONE readback (the counts): the stacked example is cut into its sectors' host fields and handed
        to ``PolarStream.sweep_to_host``; a carried list takes the first sector's metadata, as ``forward`` gives it.  'seg' / 'ins' in dataset
        order (``out['dataset_order']``: one tensor per sample, written at the ``key_points_index`` positions on the device) only need their
        token."""
        nsec = self.nsectors
        num = host_counts(cur_example["num_points"])
        bs = len(num) // nsec
        metas = cur_example.get("metadata", [None] * len(num))
        sectors = [dict(num_points=num[i * bs:(i + 1) * bs], metadata=metas[i * bs:(i + 1) * bs]) for i in range(nsec)]
        per_point = {}
        if out.get("dataset_order", False):
            per_point = {k: [{sample_token(metas, i): t} for i, t in enumerate(out[k])] for k in ("seg", "ins") if k in out}
            out = {k: v for k, v in out.items() if k not in ("seg", "ins", "dataset_order")}
        res = PolarStream.sweep_to_host(out, sectors)
        res.update(per_point)
        if per_point:
            lists = self._key_index_lists(cur_example)
            res["key_points_index"] = [self._cat_index(lists[b::bs]) for b in range(bs)]
        if isinstance(out.get("det"), dict):
            for det, meta in zip(res["det"], metas[:bs]):
                det["metadata"] = meta
        return res

    def forward(self, example, return_loss=True, **kwargs):
        """example: [previous sweep, current sweep] (polarstream.py:266-290).  ``device_only=True`` (inference): see ``_forward_device``;
        returns 'det': the last sector's device list under stateful NMS or panoptic (then with 'instances'), otherwise the list of per-sector
        device lists, and with a seg head 'seg' (under panoptic also 'ins'): the sectors' flat (rows,) int64 tensors -- or, with
        ``key_points_index`` and more than one sector, one tensor per sample in dataset order, views of one buffer, marked by
        ``'dataset_order': True``.  ``sweep_to_host`` turns that into what this method returns without the flag."""
        if isinstance(example, dict) or len(example) != 2:
            raise ValueError("PolarStreamBDCP.forward takes a list of two sweeps [previous, current]")
        if kwargs.get("device_only", False) and not return_loss and not kwargs.get("raw_preds", False) and self.test_cfg is not None:
            return self._forward_device(example, **kwargs)
        prev_sweep = self.forward_one_sweep(example[0], "feature_only", False, **kwargs)
        rets = self.forward_one_sweep(example[1], "train" if return_loss else "eval", return_loss, prev_sweep=prev_sweep, **kwargs)
        if return_loss:
            return rets
        ex = example[1]
        bs = len(ex["num_points"]) // self.nsectors
        stateful = self.test_cfg is not None and (bool(self._get("stateful_nms", False)) or self._test_flag("panoptic"))
        out = self.merge_sectors(rets, bs, stateful)
        if stateful and "det" in out:
            for det, meta in zip(out["det"], ex.get("metadata", [None] * bs)[:bs]):
                det["metadata"] = meta
        return out


@DETECTORS.register_module
class STROBE(PolarStreamBDCP):
    """STROBE (det3d/models/detectors/strobe_uber.py:12-276), the Cartesian sector-streaming baseline: ``forward`` takes the LIST of
    collated sweeps, oldest first, every sweep's sectors stacked in the batch axis (sector-major) on the first sector's Cartesian grid
    (``ops.split_cart_sectors``).  Every sweep but the last runs ``feature_only``: reader, scatter and the neck (RPNUber), then per level
    the sectors' maps are rotated and ego-warped into one whole-frame memory (``ops.cart_memory_build`` with that example's
    ``transform_matrix[:bs]``) and the memory is resampled into every sector's frame (``ops.cart_memory_read``) for the next sweep's
    memory modules -- two launches per sweep for all levels, the grids of get_grids / get_center computed inside them.  The last sweep
    runs the heads; its sectors' predictions go through ``CenterHeadSingle.predict`` (``sec_id`` / ``prev_dets`` under
    test_cfg.stateful_nms) and ``SingleConvHead.predict``, and ``merge_sectors`` puts them together.  Inference in f32 through the host API;
    training is ``train_strobe.STROBETrainStep``.
    The stacked-sweep plumbing -- canvas, per-sector slices, the per-sector predict loop -- is PolarStreamBDCP's; its polar warp, strips and
    device path are not used (``device_only`` is refused)."""

    def __init__(self, reader, backbone, neck, bbox_head, seg_head=None, part_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 nsectors=1):
        ops.cart_sector_grid((2, 2, 1), int(nsectors))      # refuses the sector counts whose grid tables are not built
        PolarStream.__init__(self, reader, backbone, neck, bbox_head, seg_head, part_head, train_cfg, test_cfg, pretrained)
        self.nsectors = int(nsectors)

    def set_compute_dtype(self, dtype: str):
        if dtype != "f32":
            raise NotImplementedError("STROBE runs in f32 only: bf16 is not built for the memory modules and the memory kernels")
        return self

    def _refuse_unbuilt(self, return_loss, **kwargs):
        eval_only(self, "STROBE")
        if return_loss:
            raise NotImplementedError("STROBE: return_loss=True is not built on the host API -- training (batch statistics, gradients through "
                                      "the memory modules, the optimizer) is train_strobe.STROBETrainStep; call forward(example_list, "
                                      "return_loss=False)")
        if kwargs.get("device_only", False):
            raise NotImplementedError("STROBE: device_only / graph capture is not built; forward(example_list, return_loss=False) is the host API")
        if self._test_flag("panoptic"):
            raise NotImplementedError("STROBE: test_cfg.panoptic (strobe_uber.py:268-273) is not built; 'det' and 'seg' are")

    def _stream_sectors(self, canvas, prev_sweep, bs, mode):
        """strobe_uber.py:111-122: all sectors of the sweep at once, the previous sweeps' maps in front of blocks i >= 1"""
        return self.neck.forward_nhwc(canvas, prev_sweep)[0]

    def update_memory(self, cur_sweep, transform, bs):
        """strobe_uber.py:172-208: per level the stacked sector maps (nsectors * bs, h, w, c) -> the map every sector reads in the next sweep,
        same shape, through the whole-frame memory.  One sector: the ego warp alone (:173-181)"""
        pr = self._get("pc_range")
        rot = torch.as_tensor(transform)[:bs]
        slots = [self.neck.prev_slot(x.shape, x.device) for x in cur_sweep]
        if self.nsectors == 1:
            return ops.cart_memory_build(cur_sweep, rot, bs, 1, pr, outs=slots)
        return ops.cart_memory_read(ops.cart_memory_build(cur_sweep, rot, bs, self.nsectors, pr), bs, self.nsectors, pr, outs=slots)

    def forward_one_sweep(self, example, mode="feature_only", return_loss=False, **kwargs):
        self._refuse_unbuilt(return_loss, **kwargs)
        if mode != "feature_only":
            return super().forward_one_sweep(example, mode, False, **kwargs)
        canvas, batch = self._canvas(example)
        _, cur = self.neck.forward_nhwc(canvas, kwargs.get("prev_sweep"))
        return self.update_memory(cur, example["transform_matrix"], batch // self.nsectors)

    def forward(self, example, return_loss=True, **kwargs):
        """example: the list of collated sweeps, oldest first (strobe_uber.py:124-142); a dict is one sweep"""
        self._refuse_unbuilt(return_loss, **kwargs)
        sweeps = [example] if isinstance(example, dict) else list(example)
        prev_sweep = None
        for ex in sweeps[:-1]:
            prev_sweep = self.forward_one_sweep(ex, "feature_only", False, prev_sweep=prev_sweep)
        ex = sweeps[-1]
        rets = self.forward_one_sweep(ex, "eval", False, **dict(kwargs, prev_sweep=prev_sweep))
        bs = len(ex["num_points"]) // self.nsectors
        stateful = self.test_cfg is not None and bool(self._get("stateful_nms", False))
        out = self.merge_sectors(rets, bs, stateful)
        if stateful and "det" in out:
            for det, meta in zip(out["det"], ex.get("metadata", [None] * bs)[:bs]):
                det["metadata"] = meta
        return out


builder.register_unbuilt(DETECTORS, "STROBEV2", "the sector-by-sector memory of strobe_uber.py:279-477 belongs, with STROBEV3, to the variants around "
                         "torchgeometry.homography_warp; STROBE is the class the reference's strobe configs name")
builder.register_unbuilt(DETECTORS, "STROBEV3", "it needs torchgeometry.homography_warp (strobe_uber.py:480-674); STROBE is the class the reference's strobe "
                         "configs name")
for _name in ("PointPillarsLSTM", "PointPillarsLSTMV1", "PointPillarsNoLSTM"):
    builder.register_unbuilt(DETECTORS, _name, "the Han detectors (streaming_waymo.py, configs/nusc/pp/han_method) are outside this build")


@DETECTORS.register_module
class VoxelNet(SingleStageDetector):
    """VoxelNet (voxelnet.py:27-131): reader -> sparse 3-D middle encoder -> RPN -> head, the detector of the reference's
    CenterPoint-style voxel configs (VoxelNetV3 is this plus the re-alignment attention).  Eval mode, on the HIP kernels."""

    def __init__(self, reader, backbone, neck, bbox_head, seg_head=None, part_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None):
        super().__init__(reader, backbone, neck, bbox_head, seg_head, part_head, train_cfg, test_cfg, pretrained)

    def extract_feat_hard(self, data, return_conv1=False):
        """voxelnet.py:47-58; returns the NHWC neck output (``return_conv1``: and the encoder's level 0, for the voxel seg head)"""
        feats = self.reader(data["features"], data["num_voxels"])
        x = self.backbone.forward_nhwc(feats, data["coors"], data["batch_size"], data["input_shape"], return_conv1=return_conv1)
        return self._through_neck(x, return_conv1)

    def extract_feat_dynamic(self, data, return_conv1=False):
        """voxelnet.py:60-70: dynamic voxel encoder (mean of the points of a voxel) -> sparse backbone on unq"""
        feats, unq = self.reader(data)
        x = self.backbone.forward_nhwc(feats, unq.to(torch.int32), data["batch_size"], [int(v) for v in data["grid_size"]], return_conv1=return_conv1)
        return self._through_neck(x, return_conv1)

    def _through_neck(self, x, with_level):
        x, level0 = x if with_level else (x, None)
        x = self.neck.forward_nhwc(x) if self.with_neck else x
        return (x, level0) if with_level else x

    def _neck_map(self, example, return_conv1=False):
        """reference ``example`` dict (hard-voxel or dynamic keys) -> the NHWC neck output (``return_conv1``: and the encoder's level 0)"""
        eval_only(self, "VoxelNet")
        if "voxels" in example:
            hip.require_device(example["voxels"], example["coordinates"])
            data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"],
                        batch_size=len(example["num_voxels"]), input_shape=[int(v) for v in example["shape"][0]])
            x = self.extract_feat_hard(data, return_conv1)
        else:
            hip.require_device(example["points"], example["grid_ind"])
            data = dict(points=example["points"], grid_ind=example["grid_ind"], num_points=example["num_points"],
                        batch_size=len(example["num_points"]), voxel_size=example["voxel_size"][0], pc_range=example["pc_range"][0],
                        grid_size=example["grid_size"][0])
            x = self.extract_feat_dynamic(data, return_conv1)
        return x

    def forward_two_stage(self, example, return_loss=False, **kwargs):
        """the first stage of a TwoStageDetector (voxelnet.py:133-168, two_stage.py:155-166), inference: whatever ``forward`` accepts ->
        (the device list of ``bbox_head.predict(device_only=True)``, the NHWC neck output); nothing is read back"""
        preds, x = self.two_stage_preds(example)
        return first_stage_device_list(self, example, preds, return_loss, **kwargs), x

    def two_stage_preds(self, example):
        """-> (the head's prediction dict, the NHWC neck output): what ``forward_two_stage`` decodes, and what ``TwoStageTrainStep`` takes the
        first stage's loss from"""
        x = self._neck_map(example)
        return self.bbox_head(ops.as_nchw(x)), x

    def forward(self, example, return_loss=True, **kwargs):
        if self.seg_head is not None:
            return self._forward_with_seg(example, return_loss, **kwargs)
        preds = self.bbox_head(ops.as_nchw(self._neck_map(example)))
        if return_loss:
            return self.bbox_head.loss(example, preds)
        if kwargs.get("raw_preds", False) or self.test_cfg is None:
            return preds
        return {"det": self.bbox_head.predict(example, preds, self.test_cfg, **kwargs)}

    def _forward_with_seg(self, example, return_loss, **kwargs):
        """voxelnet.py:72-131 with a voxel seg head (DeconvConvHead): the head reads the encoder's conv1 level and the neck's output and is
        evaluated at the active voxels -> {'seg': per-point labels} (+ 'det' with a bbox head: what the seg-less detector returns under
        that key, the raw maps without a test_cfg).  ``raw_preds``: the heads' own outputs under the two keys.  Inference."""
        if return_loss:
            raise NotImplementedError("VoxelNet: return_loss=True with a seg head is not built on the module -- the voxel segmentation head trains "
                                      "through train_voxel_seg.VoxelSegTrainStep(model, total_steps).step(example); call forward(example, return_loss=False)")
        if not hasattr(self.seg_head, "forward_voxels"):
            raise NotImplementedError(f"VoxelNet: the seg head {type(self.seg_head).__name__} has no voxel-wise form; DeconvConvHead (height > 1) is the "
                                      "seg head of the reference's VoxelNet configs")
        x, level0 = self._neck_map(example, return_conv1=True)
        seg_preds = self.seg_head.forward_voxels(level0, x)
        raw = kwargs.get("raw_preds", False)
        out = {}
        if self.bbox_head is not None:
            preds = self.bbox_head(ops.as_nchw(x))
            out["det"] = preds if (raw or self.test_cfg is None) else self.bbox_head.predict(example, preds, self.test_cfg, **kwargs)
        out["seg"] = seg_preds if raw else self.seg_head.predict(example, seg_preds, self.test_cfg, device_only=kwargs.get("device_only", False))
        return out


@DETECTORS.register_module
class VoxelNetV3(SingleStageDetector):
    """PARTNER detector (voxelnet.py:171-301): hard voxels -> mean VFE -> sparse 3-D backbone -> two SetBlocks
    (global representation re-alignment) -> RPN -> head, end to end on the HIP kernels (eval mode)."""

    def __init__(self, reader, backbone, neck, bbox_head, seg_head=None, part_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None):
        super().__init__(reader, backbone, neck, bbox_head, seg_head, part_head, train_cfg, test_cfg, pretrained)
        from .attention import SetBlock, waymo_bev_pos
        self.bev_pos = waymo_bev_pos()
        self.attns = nn.ModuleList([
            SetBlock(in_dim=256, embed_dim_scale=1, num_heads=4, reso=(144, 256), mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                     H_sp=144, W_sp=1, H=4, W=8, drop=0.1, attn_drop=0.1, drop_path=0.1, norm_layer=nn.LayerNorm,
                     pos=self.bev_pos, shift=(i % 2 == 1)) for i in range(2)])

    def set_compute_dtype(self, dtype: str) -> "VoxelNetV3":
        """"f32" (default: the reference's arithmetic, the parity path) or "bf16" (BASELINE configs[3]): the dense BEV stages on the bf16
        matrix pipe -- the RPN's and the head's convolutions (csrc/conv_bf16.hip) and the token GEMMs of the SetBlocks and of the head's
        Swin stage (pn_linear_bf16) -- with f32 accumulation; voxelization, the sparse encoder, LayerNorm / attention cores / GroupNorm,
        residual streams and every output stay f32."""
        assert dtype in ("f32", "bf16")
        # Only the LAST SetBlock: a block's output feeds the next block's key-point selection (top-4 local maxima per azimuth column, a discrete
        # choice among near-ties), and a bf16-sized perturbation of block 0's output flips enough of block 1's key points to move the head
        # tensors by 7 % of their range (measured, seeded weights) -- block 0 therefore stays f32; inside the last block the selection reads the
        # f32 LayerNorm output before any bf16 product.
        for i, attn in enumerate(self.attns):
            attn.set_compute_dtype(dtype if i == len(self.attns) - 1 else "f32")
        if self.with_neck:
            self.neck.set_compute_dtype(dtype)
        self.bbox_head.set_compute_dtype(dtype)
        if self.with_neck:
            # r6: the RPN hands its output map over in bf16 (its deblocks' epilogues round once) where the head reads it in bf16 anyway: the
            # f32 map (151 MB at bs 2) and the head's f32 -> bf16 pass over it are gone.  Same bits as rounding the f32 map.
            self.neck.bf16_output = bool(dtype == "bf16" and getattr(self.bbox_head, "takes_bf16_input", lambda: False)())
        return self

    def realign(self, x: torch.Tensor) -> torch.Tensor:
        """x: logical (B, C=256, theta=256, r=144) dense BEV map -> same shape (voxelnet.py:210-221)"""
        hip.require_device(x)
        return ops.as_nchw(self.realign_nhwc(ops.to_nhwc(x)))

    def realign_nhwc(self, xh: torch.Tensor) -> torch.Tensor:
        """NHWC (B, theta, r, C) -> same, through the two SetBlocks.  The reference permutes the map to range-major tokens and back
        (voxelnet.py:211,219); the blocks here take the tokens in the map's own azimuth-major order (``SetBlock.forward_cols``), so
        nothing is transposed -- element for element the same result (``test_setblock_column_major_equals_range_major``)."""
        b, t, r, c = xh.shape
        y = xh.contiguous().view(b, t * r, c)
        for attn in self.attns:
            y = attn.forward_cols(y)
        return y.view(b, t, r, c)

    def dense_stages_nhwc(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """the dense BEV map of the sparse backbone (B, theta, r, C) -> the head's NHWC tensors: 2 x SetBlock -> RPN -> head.
        r6: a batch of several samples runs them PER SAMPLE on two streams (branches of the same hipGraph when captured): the 2-D chain
        launches of a bs = 2 map are 576 tiles on 256 CUs -- 2.25 rounds paid as 3 --, two per-sample sequences of 288-tile launches fill
        each other's tails (tools/c4_sample_streams.py: SetBlocks + RPN + head 7.36 -> 6.99 ms).  Every kernel of these stages works on one
        sample's rows at a time, so a sample's tensors are those of the same sample alone (``PN_SAMPLE_STREAMS=0``: one sequence over the batch)."""
        def one(xs):
            y = self.realign_nhwc(xs)
            if self.with_neck:
                y = self.neck.forward_nhwc(y)
            out = self.bbox_head.forward_nhwc(y)
            out.pop("_feat", None)
            return out
        b = x.shape[0]
        if b < 2 or not R.sample_streams or not x.is_cuda:
            return one(x)
        main = torch.cuda.current_stream(x.device)
        side = ops.concurrent_stream(x.device)
        side.wait_stream(main)
        outs = [None] * b
        built = S.lazy_builds
        for i in range(0, b, 2):
            outs[i] = one(x[i:i + 1])
        if S.lazy_builds != built:      # plans / weight layouts were built on the way (the first call): they are queued on THIS stream
            side.wait_stream(main)
        with torch.cuda.stream(side):
            for i in range(1, b, 2):
                outs[i] = one(x[i:i + 1])
        main.wait_stream(side)
        for i in range(1, b, 2):
            for v in outs[i].values():
                v.record_stream(main)
        return {k: torch.cat([o[k] for o in outs], 0) for k in outs[0]}

    def extract_feat_hard(self, data):
        """voxelnet.py:202-227: mean VFE -> sparse 3-D backbone -> 2 x SetBlock -> RPN; returns the NHWC neck output"""
        feats = self.reader(data["features"], data["num_voxels"])
        x = self.backbone.forward_nhwc(feats, data["coors"], data["batch_size"], data["input_shape"])
        x = self.realign_nhwc(x)
        if self.with_neck:
            x = self.neck.forward_nhwc(x)
        return x

    def forward_points(self, points: torch.Tensor, voxel_generator=None, sample_offsets=None):
        """Fused path from polar-decorated points (N, F) on the device: hard voxelization (device, count stays on the device) -> mean VFE
        -> sparse backbone -> 2 x SetBlock -> RPN -> head.  No host synchronisation: capturable in a hipGraph (``engine.FrameEngine``).
        ``voxel_generator``: dict(range, voxel_size, max_points_in_voxel, max_voxel_num); default = the one the config hands to the head.
        ``sample_offsets``: python ints [0, n_0, n_0 + n_1, ...] for a batch of several sweeps (r3): every sample is voxelized on its own
        and the lists are joined on the device (pn_concat_voxel_segments_f32 = the reference's collate, counts included)."""
        eval_only(self, "VoxelNetV3")
        vg = voxel_generator or getattr(self.bbox_head, "voxel_generator_cfg", None)
        if vg is None:
            raise ValueError("VoxelNetV3.forward_points needs the voxel_generator section of the config")
        mv = vg["max_voxel_num"]
        mv = int(mv[0] if isinstance(mv, (list, tuple)) else mv)
        rg, vs = vg["range"], vg["voxel_size"]
        grid = [int(round((rg[3 + a] - rg[a]) / vs[a])) for a in range(3)]
        offs = [0, int(points.shape[0])] if sample_offsets is None else [int(v) for v in sample_offsets]
        batch = len(offs) - 1
        if batch == 1:
            voxels, coors, num, nv = ops.hard_voxelize(points, vg["voxel_size"], vg["range"], int(vg["max_points_in_voxel"]), mv)
            feats = self.reader(voxels, num)
            coords4 = torch.cat([torch.zeros((mv, 1), dtype=torch.int32, device=points.device), coors], 1)
        else:
            fs, cs, nvs = [], [], []
            for b in range(batch):
                voxels, coors, num, nv = ops.hard_voxelize(points[offs[b]:offs[b + 1]], vg["voxel_size"], vg["range"], int(vg["max_points_in_voxel"]), mv)
                fs.append(self.reader(voxels, num))
                cs.append(coors)
                nvs.append(nv)
            seg_f, seg_c, counts = torch.stack(fs).contiguous(), torch.stack(cs).contiguous(), torch.cat(nvs).contiguous()
            feats = torch.zeros((batch * mv, seg_f.shape[2]), dtype=torch.float32, device=points.device)
            coords4 = torch.zeros((batch * mv, 4), dtype=torch.int32, device=points.device)
            nv = torch.empty((1,), dtype=torch.int32, device=points.device)
            hip.call("pn_concat_voxel_segments_f32", seg_f.data_ptr(), seg_c.data_ptr(), counts.data_ptr(), batch, mv, int(seg_f.shape[2]),
                     feats.data_ptr(), coords4.data_ptr(), nv.data_ptr(), hip.stream())
        out = self.dense_stages_nhwc(self.backbone.forward_nhwc(feats, coords4, batch, grid, n_voxels=nv))
        return {k: v.permute(0, 3, 1, 2) for k, v in out.items()}

    def extract_feat_dynamic(self, data):
        """voxelnet.py:228-237: dynamic voxel encoder -> sparse backbone on unq -> RPN.  As in the reference this branch does NOT pass through
        the re-alignment attention (only ``extract_feat_hard`` does); returns the NHWC neck output"""
        feats, unq = self.reader(data)
        x = self.backbone.forward_nhwc(feats, unq.to(torch.int32), data["batch_size"], [int(v) for v in data["grid_size"]])
        return self.neck.forward_nhwc(x) if self.with_neck else x

    def forward(self, example, return_loss=True, **kwargs):
        """voxelnet.py:239-301.  Hard-voxel branch (the Waymo PARTNER config): example keys voxels (V,P,F), coordinates (V,4) [b,z,y,x],
        num_points (V,), num_voxels (B,), shape [[x,y,z]]; dynamic branch (r6): points, grid_ind, num_points, voxel_size, pc_range, grid_size"""
        if "voxels" not in example:
            hip.require_device(example["points"], example["grid_ind"])
            data = dict(points=example["points"], grid_ind=example["grid_ind"], num_points=example["num_points"],
                        batch_size=len(example["num_points"]), voxel_size=example["voxel_size"][0], pc_range=example["pc_range"][0],
                        grid_size=example["grid_size"][0])
            x = self.extract_feat_dynamic(data)
        else:
            hip.require_device(example["voxels"], example["coordinates"])
            data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"],
                        batch_size=len(example["num_voxels"]), input_shape=[int(v) for v in example["shape"][0]])
            x = None
        if x is None and hasattr(self.bbox_head, "forward_nhwc"):
            feats = self.reader(data["features"], data["num_voxels"])
            head_out = self.dense_stages_nhwc(self.backbone.forward_nhwc(feats, data["coors"], data["batch_size"], data["input_shape"]))
        else:
            x = self.extract_feat_hard(data) if x is None else x
            head_out = self.bbox_head.forward_nhwc(x) if hasattr(self.bbox_head, "forward_nhwc") else None
        if head_out is not None:
            head_out.pop("_feat", None)
            preds = {"det_preds": [{k: v.permute(0, 3, 1, 2) for k, v in head_out.items()}]}
        else:
            preds = self.bbox_head(ops.as_nchw(x))
        if return_loss:
            return self.bbox_head.loss(example, preds)
        if kwargs.get("raw_preds", False) or self.test_cfg is None:
            return preds
        return {"det": self.bbox_head.predict(example, preds, self.test_cfg, **kwargs)}
