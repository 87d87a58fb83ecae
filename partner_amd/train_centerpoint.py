"""One training iteration of the plain CenterPoint detectors, the ones most of the reference's configs build:

  VoxelNet      VoxelFeatureExtractorV3 / DynamicVoxelEncoderV1 -> SpMiddleResNetFHD -> RPN -> CenterHead
                (configs/nusc/voxelnet/nusc_centerpoint_voxelnet_01voxel.py, ..._0075voxel_dcn*.py, configs/waymo/voxelnet/waymo_centerpoint_voxelnet_*.py)
  PointPillars  PillarFeatureNet -> PointPillarsScatter -> RPN -> CenterHead
                (configs/waymo/pp/waymo_centerpoint_pp_two_pfn_stride1_3x.py and its two-class twin)

Reference call stack of the iteration: det3d/torchie/trainer/trainer.py:275-300 (batch_processor -> model(example, return_loss=True) ->
loss.backward() -> optimizer hooks), det3d/models/detectors/voxelnet.py:72-131 / point_pillars.py:27-96 (forward),
det3d/models/bbox_heads/center_head.py:248-288 (loss), det3d/solver/fastai_optim.py:155-171 (OneCycle Adam with decoupled weight decay),
det3d/torchie/trainer/hooks/optimizer.py:10-13 (clip_grad_norm_ 35).

The encoder and the RPN run on the reverse-mode tape of autodiff.py (sparse_train / train_partner.rpn_train), the head is the part of the
other detection steps (train_head.CenterHeadTrain: plain multi-task head, dcn_head=True included) and the hard-voxel reader's training form
is csrc/pfn_static_train.hip: its backward takes the canvas gradient the tape leaves and gathers the pillars' rows itself.  All arithmetic is
HIP kernels; BatchNorm layers use batch statistics and update their running buffers."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import autodiff as ad
from . import hip, ops
from .readers import DynamicPFNet, PillarFeatureNet
from .sparse_train import sp_middle_resnet_fhd_train
from .train import FlatAdam, OptimizerForwards, ParamStore
from .train_head import CenterHeadTrain
from .train_partner import rpn_train

LOSS_KEYS = ("det_loss", "hm_loss", "loc_loss", "loc_loss_elem", "num_positive")      # CenterHead.loss (center_head.py:276-288)


class CenterPointTrainStep(OptimizerForwards):
    """``step(example)``: forward (training mode), the CenterPoint loss of every task, backward, gradient all-reduce (when torch.distributed
    runs with world_size > 1), clip + decoupled weight decay + Adam under the OneCycle schedule.  ``example``: the reference's collated dict on
    the device -- the hard-voxel keys (voxels (V,P,F), coordinates (V,4) [b,z,y,x], num_points (V,), num_voxels (B,), shape [[x,y,z]]), or for a
    VoxelNet with DynamicVoxelEncoderV1 the dynamic keys -- and the assigner's per-task lists hm, anno_box, ind, mask, cat.
    -> the dict of ``CenterHead.loss``: one device tensor per task under each key.  Nothing is read back."""

    def __init__(self, model: nn.Module, total_steps: int, lr_max=0.003, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4, weight_decay=0.01,
                 max_norm=35.0, beta2=0.99, eps=1e-8):
        kind = type(model).__name__
        if kind == "VoxelNetV3":
            raise NotImplementedError("CenterPointTrainStep: VoxelNetV3 (the re-alignment attention) trains through train_partner.PartnerTrainStep")
        if getattr(model, "seg_head", None) is not None:
            raise NotImplementedError("CenterPointTrainStep: the detector has a seg_head -- the joint det + seg step is not built; the voxel seg head "
                                      "trains alone through train_voxel_seg.VoxelSegTrainStep, the pillar seg head with the polar-pillar model "
                                      "through train.PolarPillarTrainStep")
        for attr in ("reader", "backbone", "neck", "bbox_head"):
            if getattr(model, attr, None) is None:
                raise NotImplementedError(f"CenterPointTrainStep: the detector has no `{attr}` (expected VoxelNet or PointPillars)")
        if isinstance(model.reader, DynamicPFNet):
            raise NotImplementedError("CenterPointTrainStep: a DynamicPFNet reader trains through train.PolarPillarTrainStep")
        if type(model.bbox_head).__name__ != "CenterHead":
            raise NotImplementedError(f"CenterPointTrainStep: the head is a {type(model.bbox_head).__name__}, not the plain CenterHead (the merged "
                                      "heads train with the polar-pillar model, the set head through PartnerTrainStep)")
        if any(p.dtype != torch.float32 for p in model.parameters()) or getattr(model, "compute_dtype", "f32") != "f32":
            raise NotImplementedError("CenterPointTrainStep: bf16 is not built -- the plain CenterPoint detectors train in f32 only")
        self.pillars = isinstance(model.reader, PillarFeatureNet)
        if self.pillars:
            if len(model.reader.pfn_layers) > 2:
                raise NotImplementedError("CenterPointTrainStep: more than two PFN layers -- the reader's training kernels (csrc/pfn_static_train.hip) "
                                          "take one or two")
        elif any(True for _ in model.reader.parameters()):
            raise NotImplementedError(f"CenterPointTrainStep: the reader {type(model.reader).__name__} has parameters -- PillarFeatureNet, "
                                      "VoxelFeatureExtractorV3 and DynamicVoxelEncoderV1 are taken")
        if not model.training:
            raise ValueError("CenterPointTrainStep: the model must be in train mode (BatchNorm uses batch statistics)")
        self.model = model
        p0 = next(model.parameters())
        hip.require_device(p0)
        self.dev = p0.device
        self.ps = ParamStore(model, self.dev)
        self.opt = FlatAdam(self.ps, model, total_steps, lr_max, moms, div_factor, pct_start, weight_decay, max_norm, beta2, eps)
        self.head_train = CenterHeadTrain(self.ps, model.bbox_head, self.dev)
        self.last_tape: Optional[ad.Tape] = None

    # ------------------------------------------------------------------------------------------
    def _encoder_inputs(self, example):
        """VoxelNet: the reader's output and the encoder's coordinates (train_voxel_seg.VoxelSegTrainStep._encoder_inputs)"""
        m = self.model
        if "voxels" in example:
            hip.require_device(example["voxels"], example["coordinates"])
            feats = m.reader(example["voxels"], example["num_points"])
            return feats, example["coordinates"], len(example["num_voxels"]), [int(v) for v in example["shape"][0]]
        hip.require_device(example["points"], example["grid_ind"])
        data = dict(points=example["points"], grid_ind=example["grid_ind"], num_points=example["num_points"], batch_size=len(example["num_points"]),
                    voxel_size=example["voxel_size"][0], pc_range=example["pc_range"][0], grid_size=example["grid_size"][0])
        feats, unq = m.reader(data)
        return feats, unq.to(torch.int32), data["batch_size"], [int(v) for v in data["grid_size"]]

    def _pfn_layers(self):
        return [(layer.linear.weight.data, layer.norm) for layer in self.model.reader.pfn_layers]

    def _targets(self, example):
        n = len(self.model.bbox_head.tasks)
        for k in ("hm", "anno_box", "ind", "mask", "cat"):
            if k not in example or len(example[k]) != n:
                raise ValueError(f"CenterPointTrainStep: example['{k}'] must hold one entry per task ({n})")
        return [ops.CenterLossTargets(example["hm"][t], example["ind"][t], example["mask"][t], example["cat"][t], example["anno_box"][t], self.dev)
                for t in range(n)]

    def forward_backward(self, example, grad_scale=1.0):
        """forward + loss + backward; the gradients land in ``self.ps.flat_g`` (overwritten).  -> the loss dict of the head"""
        m, ps = self.model, self.ps
        targets = self._targets(example)
        t = ad.Tape()
        reader_bwd = None
        if self.pillars:
            r = m.reader
            vox, coors = example["voxels"], example["coordinates"]
            hip.require_device(vox, coors)
            vox, coors = vox.contiguous(), coors.to(torch.int32).contiguous()
            num = example["num_points"].to(torch.int32).contiguous()
            batch, shape = len(example["num_voxels"]), [int(v) for v in example["shape"][0]]
            geo = dict(vx=float(r.vx), vy=float(r.vy), x_offset=float(r.x_offset), y_offset=float(r.y_offset), with_distance=r._with_distance)
            layers = self._pfn_layers()
            feats, saved = ops.static_pfn_train(vox, num, coors, layers, **geo)
            canvas = t.input(ops.scatter_canvas(feats, coors.to(torch.int64), batch, shape[1], shape[0]))
            x = canvas

            def reader_bwd():
                names = [f"reader.pfn_layers.{i}.{k}" for i in range(len(layers)) for k in ("linear.weight", "norm.weight", "norm.bias")]
                ops.static_pfn_train_bwd(vox, num, coors, layers, saved=saved, d_canvas=canvas.g.contiguous(), out=[ps.g[n] for n in names], **geo)
        else:
            feats, coors, batch, shape = self._encoder_inputs(example)
            x = sp_middle_resnet_fhd_train(t, m.backbone, feats, coors, batch, shape, prefix="backbone.")
        if getattr(m, "with_neck", m.neck is not None):
            x = rpn_train(t, m.neck, x)
        hip.call("pn_fill_zero", ps.flat_g.data_ptr(), ps.flat_g.numel() * 4, hip.stream())
        ht = self.head_train
        ht.forward(x.v)
        losses = ht.losses(targets)
        ad.accumulate(x, ht.backward(targets, losses, grad_scale))
        ps.side.join()      # the head's weight gradients (the side stream) are in flat_g
        t.backward()
        # parameter gradients of the tape into the flat buffer; the head's and the reader's kernels write their ranges themselves
        for leaf in t.params:
            if leaf.g is not None:
                ops.add(ps.g[leaf.name].view(-1), leaf.g.contiguous().view(-1), out=ps.g[leaf.name].view(-1))
        if reader_bwd is not None:
            reader_bwd()
        self.last_tape = t
        out = {k: [] for k in LOSS_KEYS}
        for lo in losses:      # the kernel's vector: [det, hm, loc, num_pos, elem...]
            out["det_loss"].append(lo[0])
            out["hm_loss"].append(lo[1])
            out["loc_loss"].append(lo[2])
            out["loc_loss_elem"].append(lo[4:])
            out["num_positive"].append(lo[3])
        return out

    def sync_initial_params(self):
        self.opt.sync_initial_params()

    def step(self, example):
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        losses = self.forward_backward(example, grad_scale=1.0 / world)
        if world > 1:
            from .dist_utils import GradExchange
            ex = GradExchange(self.ps.flat_g, [(0, self.ps.total)])
            ex.ready(0)
            ex.finish()
        self.optimizer_step()
        return losses
