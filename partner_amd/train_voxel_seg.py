"""Training the voxel-wise segmentation head (DeconvConvHead with height > 1, det3d/models/seg_heads/seg_head.py:195-264 with ``loss``,
:86-96, under autograd in the reference; configs/nusc/voxelnet/voxelnet_seg_cylinder.py).

The dense form would hold a 1 GB logit tensor per sample and its gradient; the reference's loss reads the dense logits only at the
labelled cells (``ignore=-1`` after ``get_labels``' ``labels - 1``).  So the head is evaluated at the labelled cells
(``ops.voxel_seg_label_queries``), the loss is ``weight * SegLoss`` over those rows (``seg_heads.seg_loss_nhwc``), and backward runs over
the same list (csrc/voxel_seg.hip: pn_voxel_seg_wgrad_f32 / _dfeat_f32 / _du_f32, pn_deconv_overlap_bwd_f32).  Labelled cells need not be
active sites: the dense reference predicts there too.

  voxel_seg_head_train   the head on the tape of autodiff.py
  voxel_seg_loss         labels -> query list -> head -> loss -> the seed of backward
  VoxelSegTrainStep      one iteration of a seg-only VoxelNet: reader -> SpMiddleResNetFHD -> RPN -> head at the labelled cells -> FlatAdam
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import autodiff as ad
from . import hip, ops
from .seg_heads import DeconvConvHead, seg_loss_nhwc
from .sparse_train import sp_middle_resnet_fhd_train
from .train import FlatAdam, OptimizerForwards, ParamStore
from .train_partner import rpn_train


def voxel_seg_head_train(t: ad.Tape, head: DeconvConvHead, conv1_node: ad.Node, level0, x2_node: ad.Node, queries: torch.Tensor,
                         n_queries: torch.Tensor, prefix="seg_head.") -> ad.Node:
    """``DeconvConvHead.forward`` at the cells ``queries`` (int32 keys of ``level0.dims``, UNIQUE and strictly ASCENDING, ``n_queries`` their
    device count) on the tape -> the logits node (rows, NCpad); rows at or beyond the count are zeros.  conv1_node: the (n, 16) rows of
    ``level0``; x2_node: the neck's NHWC output (B, h, w, Cin).  The three parameters are tape leaves under their state-dict names; the packed
    weights are rebuilt from the leaves on every call.  Backward accumulates into conv1_node, x2_node and the three leaves."""
    hip.require_device(conv1_node.v, x2_node.v, queries, n_queries)
    wd = t.param(head.deconv.weight.data, prefix + "deconv.weight")
    wc = t.param(head.conv.weight.data, prefix + "conv.weight")
    bc = t.param(head.conv.bias.data, prefix + "conv.bias")
    s, d, nc = head.up_scale, head.height, head.num_classes
    b, dd, h, w = level0.dims
    if dd != d:
        raise ValueError(f"voxel_seg_head_train: the level is {dd} cells high, the head was built with height {d}")
    bb, hh, ww, cin = x2_node.v.shape
    if (bb, hh * s, ww * s) != (b, h, w):
        raise ValueError(f"voxel_seg_head_train: the neck map {(hh, ww)} times up_scale {s} is not the voxel level {(h, w)}")
    assert conv1_node.v.shape[1] == 16 and conv1_node.v.is_contiguous()
    level = ops.SparseLevel(feats=conv1_node.v, index=level0.index, keys=level0.keys, count=level0.count, cap=int(conv1_node.v.shape[0]),
                            dims=list(level0.dims))

    # the transposed convolution: one GEMM (ad.linear gives its data and weight gradients) and the overlap-add
    wm_v = wd.v.permute(2, 3, 1, 0).reshape(4 * s * s * d, cin).contiguous()      # row (ky 2S + kx) D + c

    def wm_bw(g):      # on the stream the GEMM's weight gradient was queued on
        ad.side_run(lambda: ad.accumulate(wd, g.view(2 * s, 2 * s, d, cin).permute(3, 2, 0, 1).contiguous(), own=True), g)

    wm = t.new(wm_v, wm_bw)
    cols = ad.linear(t, ad.view(t, x2_node, (bb * hh * ww, cin)), wm, None)
    u_v = torch.empty((b, h, w, d), dtype=torch.float32, device=cols.v.device)
    hip.call("pn_deconv_overlap_f32", cols.v.data_ptr(), bb, hh, ww, s, d, u_v.data_ptr(), hip.stream())
    u = t.new(u_v, lambda g: ad.accumulate(cols, ops.deconv_overlap_bwd(g.contiguous(), s), own=True))

    packed, pbias = ops.voxel_seg_pack(wc.v, bc.v, d, nc)
    ncp = ops.voxel_seg_class_pad(nc)
    logits = torch.zeros((int(queries.shape[0]), ncp), dtype=torch.float32, device=u_v.device)
    ops.voxel_seg_logits(level, u_v, packed, pbias, nc, queries, n_queries, out=logits)

    def bw(g):
        g = g.contiguous()
        qindex = ops.voxel_seg_query_index(queries, n_queries, level.dims)
        d_packed, d_pbias = ops.voxel_seg_wgrad(level, u_v, queries, n_queries, g, nc)
        gw, gb = ops.voxel_seg_unpack_grads(d_packed, d_pbias, d, nc)
        ad.accumulate(wc, gw.contiguous(), own=True)
        ad.accumulate(bc, gb, own=True)
        ad.accumulate(conv1_node, ops.voxel_seg_dfeat(level, qindex, g, packed, nc), own=True)
        ad.accumulate(u, ops.voxel_seg_du(level.dims, qindex, g, packed, nc), own=True)

    return t.new(logits, bw)


def voxel_seg_loss(t: ad.Tape, head: DeconvConvHead, conv1_node: ad.Node, level0, x2_node: ad.Node, voxel_labels: torch.Tensor,
                   capacity: Optional[int] = None, scale: float = 1.0, prefix="seg_head."):
    """``DeconvConvHead.loss`` (seg_head.py:86-96) on the tape: the labelled cells of ``voxel_labels`` (device, (B, D, H, W) or (B, 1, D, H, W))
    become the query list, the head is evaluated there, ``weight * SegLoss(ignore=-1)`` runs over those rows and its gradient (times
    ``scale``) seeds the logits node.  ``capacity``: rows of the list (default: every cell) -- a step passes a bound on the labelled cells.
    -> (loss vector (5,) [loss, lovasz, ce, n_valid, n_present] of SegLoss itself (the head's ``weight`` multiplies the gradient, and the
    caller's reported value), status (2,) int32 [list overflow, loss overflow], logits node).
    The loss reads a row only where its label is a class, so rows behind the count (label -1) are never read; no valid cell gives loss 0
    and a zero gradient, as the pillar seg loss documents."""
    if not voxel_labels.is_cuda:
        raise NotImplementedError("voxel_seg_loss: voxel_labels on the host -- the labelled-cell list is built on the device (pn_voxel_seg_label_queries)")
    lab = voxel_labels[:, 0] if voxel_labels.dim() == 5 else voxel_labels
    if [int(v) for v in lab.shape] != [int(v) for v in level0.dims]:
        raise ValueError(f"voxel_seg_loss: voxel_labels {tuple(lab.shape)} against the voxel level {tuple(level0.dims)} -- the pooled branch of get_labels "
                         "does not apply to the voxel-wise head")
    cap = int(capacity) if capacity is not None else lab.numel()
    keys, rows, count, st_list = ops.voxel_seg_label_queries(lab, head.num_classes, cap)
    logits = voxel_seg_head_train(t, head, conv1_node, level0, x2_node, keys, count, prefix)
    ncp = logits.v.shape[1]
    ignore = getattr(head.loss_func, "ignore", -1)
    vec, dlogits, st_loss = seg_loss_nhwc(logits.v, ncp, head.num_classes, rows, ignore, scale=float(head.weight) * float(scale), max_valid=cap)
    ad.accumulate(logits, dlogits)
    return vec, torch.cat([st_list, st_loss]), logits


class VoxelSegTrainStep(OptimizerForwards):
    """``step(example)``: one training iteration of a seg-only VoxelNet (voxelnet.py:72-131 with ``seg_head`` = DeconvConvHead and no
    ``bbox_head``; trainer.py:275-300; fastai_optim.py:155-171): reader -> SpMiddleResNetFHD (BatchNorm batch statistics) -> RPN -> the head
    at the labelled cells -> ``weight * SegLoss`` -> backward -> clip + decoupled weight decay + Adam under the OneCycle schedule, with the
    gradient exchange of the other steps when torch.distributed runs with world_size > 1.  ``example``: the hard-voxel keys with
    ``VoxelFeatureExtractorV3`` or the dynamic keys with ``DynamicVoxelEncoderV1`` (both readers have no parameters), plus
    ``voxel_labels`` on the device.  -> {'seg_loss': [device scalar]}.  Nothing is read back beyond the encoder's level counts."""

    def __init__(self, model: nn.Module, total_steps: int, lr_max=0.003, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4, weight_decay=0.01,
                 max_norm=35.0, beta2=0.99, eps=1e-8, max_labelled: Optional[int] = None):
        if getattr(model, "bbox_head", None) is not None:
            raise NotImplementedError("VoxelSegTrainStep: the detector has a bbox_head -- a joint det + seg step needs the plain-VoxelNet detection "
                                      "training step, which is not built; train the seg head on a VoxelNet with bbox_head=None")
        if not isinstance(getattr(model, "seg_head", None), DeconvConvHead):
            raise NotImplementedError("VoxelSegTrainStep: the detector's seg_head is not a DeconvConvHead (height > 1)")
        for attr in ("reader", "backbone", "neck"):
            if getattr(model, attr, None) is None:
                raise NotImplementedError(f"VoxelSegTrainStep: the detector has no `{attr}` (expected VoxelNet)")
        if any(True for _ in model.reader.parameters()):
            raise NotImplementedError("VoxelSegTrainStep: a reader with parameters -- VoxelFeatureExtractorV3 and DynamicVoxelEncoderV1 are taken")
        if any(p.dtype != torch.float32 for p in model.parameters()) or getattr(model, "compute_dtype", "f32") != "f32":
            raise NotImplementedError("VoxelSegTrainStep: bf16 is not built -- the voxel-wise head trains in f32 only")
        if not model.training:
            raise ValueError("VoxelSegTrainStep: the model must be in train mode (BatchNorm uses batch statistics)")
        self.model = model
        p0 = next(model.parameters())
        hip.require_device(p0)
        self.dev = p0.device
        self.ps = ParamStore(model, self.dev)
        self.opt = FlatAdam(self.ps, model, total_steps, lr_max, moms, div_factor, pct_start, weight_decay, max_norm, beta2, eps)
        self.max_labelled = max_labelled
        self.last_tape: Optional[ad.Tape] = None
        self.last_status: Optional[torch.Tensor] = None

    def _encoder_inputs(self, example):
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

    def forward_backward(self, example, grad_scale=1.0):
        """forward + loss + backward; the gradients land in ``self.ps.flat_g`` (overwritten) -> {'seg_loss': [device scalar]}"""
        m = self.model
        labels = example["voxel_labels"]
        if not torch.is_tensor(labels) or not labels.is_cuda:
            raise NotImplementedError("VoxelSegTrainStep: example['voxel_labels'] on the host -- the labelled-cell list is built on the device")
        feats, coors, batch, shape = self._encoder_inputs(example)
        t = ad.Tape()
        x, conv1, level0 = sp_middle_resnet_fhd_train(t, m.backbone, feats, coors, batch, shape, prefix="backbone.", return_conv1=True)
        if getattr(m, "with_neck", m.neck is not None):
            x = rpn_train(t, m.neck, x)
        vec, status, _ = voxel_seg_loss(t, m.seg_head, conv1, level0, x, labels, capacity=self.max_labelled, scale=grad_scale)
        t.backward()
        hip.call("pn_fill_zero", self.ps.flat_g.data_ptr(), self.ps.flat_g.numel() * 4, hip.stream())
        for leaf in t.params:
            if leaf.g is not None:
                ops.add(self.ps.g[leaf.name].view(-1), leaf.g.contiguous().view(-1), out=self.ps.g[leaf.name].view(-1))
        self.last_tape, self.last_status = t, status
        w = float(m.seg_head.weight)
        return {"seg_loss": [vec[0] if w == 1.0 else vec[0] * w]}

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
