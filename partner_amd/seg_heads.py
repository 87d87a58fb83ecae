"""Segmentation head of the reference's nuScenes polar config (`super_tasks = ['det', 'seg']`): SingleConvHead
(det3d/models/seg_heads/seg_head.py:53-96, 99-168, 176-195), its label helper ``get_labels`` (seg_head.py:24-49) and its loss object
SegLoss (det3d/models/losses/seg_loss.py:8-22).  Secondary to the detection hot path.  Forward, per-point prediction and the panoptic
fusion with the detection boxes run on the HIP kernels (eval).  Training: SegLoss = Lovasz softmax + cross entropy with its gradient
(csrc/seg_loss.hip: device-resident compaction, segmented radix sort, integer scans; nothing is read back), ``SingleConvHead.loss``, and
``SegHeadTrain``, the head's explicit forward / backward (1x1 convolutions, the bilinear up-sampling and its adjoint) that
``train.PolarPillarTrainStep`` drives.  The targets: ``ops.voxel_labels_from_points`` (the dataset's per-cell majority vote) and the
pooled down-sampling branch of ``get_labels`` (seg_head.py:33-49), both on csrc/seg_labels.hip."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch
from torch import nn

from . import builder, hip, ops
from .builder import LOSSES, SEG_HEAD
from .nn_utils import PlanCache, eval_only

# the ten nuScenes lidarseg thing classes in label order (semantic labels 1..10) under their detection class names
# (the module constant `semantic2box`, seg_head.py:11-22)
SEMANTIC2BOX = ["barrier", "bicycle", "bus", "car", "construction_vehicle", "motorcycle", "pedestrian", "traffic_cone", "trailer", "truck"]


def host_counts(num) -> list:
    """per-sample counts (``example['num_points']``: a list, an array or a tensor) as host ints"""
    return [int(v) for v in (num.tolist() if torch.is_tensor(num) else num)]


def prefix_sums(counts) -> list:
    """exclusive prefix sums of ``counts``, the total last: (len(counts) + 1) entries"""
    acc = [0]
    for v in counts:
        acc.append(acc[-1] + v)
    return acc


def device_offsets(example, key, acc, dev) -> torch.Tensor:
    """``example[key]`` when present, otherwise the host prefix sums ``acc`` as a device int32 tensor, built once and kept in the
    example under ``key`` (an upload: not capturable)"""
    offs = example.get(key)
    if offs is None:
        offs = example[key] = torch.tensor(acc, dtype=torch.int32, device=dev)
    hip.require_device(offs)
    return offs


def sample_token(metas, i):
    """the key of sample i's per-point outputs: its metadata's token, or its position"""
    meta = metas[i]
    return meta["token"] if isinstance(meta, dict) and "token" in meta else i


def merge_per_token(sectors, batch_size) -> list:
    """per-sample {token: tensor} dicts of the sectors, in sector order -> per sample one dict, every token's tensors concatenated
    (single_stage.py:106-116)"""
    merged = [{} for _ in range(batch_size)]
    for sec in sectors:
        for i in range(batch_size):
            for token, v in sec[i].items():
                merged[i].setdefault(token, []).append(v)
    return [{token: torch.cat(v) for token, v in m.items()} for m in merged]


def seg_loss_sizes() -> dict:
    """the sizes at which the loss kernels change path: keys per tile of the compaction / radix sort / scan, threads per block, keys ranked
    per step of the radix scatter (one wave)"""
    lib = hip.load()
    return dict(tile=lib.pn_seg_loss_tile_elems(0), block=lib.pn_seg_loss_tile_elems(1), chunk=lib.pn_seg_loss_tile_elems(2))


class PooledLabelsOnHost(hip.PartnerHipError, NotImplementedError):
    """host labels reached the pooled branch of ``get_labels``: like every operator it has no CPU fallback (PartnerHipError); callers that
    probed the branch before it existed keep seeing the NotImplementedError it used to raise for them"""


def get_labels(labels: torch.Tensor, pred_shape) -> torch.Tensor:
    """semantic labels for the loss from ``voxel_labels`` (0 = unlabelled): equal shapes -> ``labels - 1`` (seg_head.py:30-32; hence the
    config's ``ignore=-1``).  Labels larger than the prediction (seg_head.py:33-49) are pooled on the device (`pn_pool_labels`): per
    window of (kh, kw, kl) = floor(label shape / prediction shape) cells -- kh = Z for (B,Z,H,W) labels against a 2-D prediction -- the
    most frequent label among 1..255 minus one, the lowest among equals, -1 for a window without one; int64, (B, H // kw, W // kl) or
    (B, Z // kh, H // kw, W // kl) (rows / columns that do not fill a window are dropped, as AvgPool does)."""
    label_shape, pred_shape = tuple(labels.shape[1:]), tuple(pred_shape)
    if label_shape == pred_shape:
        return labels - 1
    if len(label_shape) not in (2, 3) or len(pred_shape) not in (2, 3) or len(pred_shape) > len(label_shape):
        raise ValueError(f"get_labels: labels {label_shape} against predictions {pred_shape}")
    kw, kl = label_shape[-2] // pred_shape[-2], label_shape[-1] // pred_shape[-1]
    kh = 1 if len(label_shape) == 2 else (label_shape[0] if len(pred_shape) == 2 else label_shape[0] // pred_shape[0])
    if min(kh, kw, kl) < 1:
        raise ValueError(f"get_labels: labels {label_shape} are smaller than the predictions {pred_shape}")
    if not labels.is_cuda:
        raise PooledLabelsOnHost(f"get_labels: labels {label_shape} against predictions {pred_shape} -- the pooled down-sampling branch of "
                                 "get_labels (seg_head.py:33-49) is built for device tensors only (pn_pool_labels); there is no host path")
    if labels.dtype not in (torch.uint8, torch.int32, torch.int64):
        labels = labels.to(torch.int64)
    out = ops.pool_labels(labels if labels.dim() == 4 else labels.unsqueeze(1), kh, kw, kl)
    return out.squeeze(1)       # a single plane is dropped, as the reference's squeeze(-3) does


def seg_loss_nhwc(logits: torch.Tensor, pixel_stride: int, num_classes: int, labels: torch.Tensor, ignore: int, scale: float = 1.0,
                  max_valid: Optional[int] = None, want_grad: bool = True):
    """`pn_seg_loss_f32` on logits stored as rows of ``pixel_stride`` floats per cell (an NHWC buffer with padded channels, read in
    place; ``logits`` is any tensor whose data pointer is the first row).  labels: device int32 / int64, one per cell in (b, y, x) order.
    -> (vec (5,) [loss, lovasz, ce, n_valid, n_present], dlogits (cells, pixel_stride) = d(scale * loss)/d(logits) or None,
    status (1,) int32: 1 when more than ``max_valid`` cells are labelled).  All on the device, nothing is read back."""
    hip.require_device(logits, labels)
    assert logits.dtype == torch.float32
    if labels.dtype not in (torch.int32, torch.int64):
        labels = labels.to(torch.int64)
    labels = labels.contiguous()
    cells = labels.numel()
    dev = logits.device
    lib = hip.load()
    cap = int(max_valid) if max_valid is not None else 0
    nbytes = lib.pn_seg_loss_workspace_bytes(cells, num_classes, cap)
    if nbytes == 0:
        raise hip.PartnerHipError(f"seg_loss: unsupported sizes (cells {cells}, classes {num_classes})")
    ws = ops._workspace(nbytes, dev)
    vec = torch.empty(5, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    dlogits = torch.empty((cells, pixel_stride), dtype=torch.float32, device=dev) if want_grad else None
    hip.call("pn_seg_loss_f32", logits.data_ptr(), int(pixel_stride), cells, int(num_classes), labels.data_ptr(), int(labels.dtype == torch.int64),
             int(ignore), cap, float(scale), vec.data_ptr(), status.data_ptr(), hip.ptr(dlogits), ws.data_ptr(), nbytes, hip.stream())
    return vec, dlogits, status


def bilinear_upsample_add_bwd(d_out: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """d_low (B,h,w,C) = adjoint of ``pn_bilinear_upsample_add_f32`` applied to d_out (B,H,W,C) NHWC, C a multiple of 4"""
    hip.require_device(d_out)
    assert d_out.dim() == 4 and d_out.is_contiguous() and d_out.dtype == torch.float32
    b, hh, ww, c = d_out.shape
    d_low = torch.empty((b, h, w, c), dtype=torch.float32, device=d_out.device)
    hip.call("pn_bilinear_upsample_add_bwd_f32", d_out.data_ptr(), b, h, w, c, hh, ww, d_low.data_ptr(), hip.stream())
    return d_low


@LOSSES.register_module
class SegLoss(nn.Module):
    """lovasz_softmax(softmax(outputs), labels, ignore) + CrossEntropyLoss(ignore_index=ignore) (seg_loss.py:19-22), parameter-free.

    Departures from the reference, which is broken there: no valid cell -> loss 0 and a zero gradient (the reference returns an empty
    tensor + NaN); one valid cell -> the formula is evaluated (the reference raises in flatten_probas).  Equal errors are ordered by
    ascending cell index (the reference's torch.sort is unstable)."""

    def __init__(self, ignore=0):
        super().__init__()
        self.ignore = ignore

    @staticmethod
    def _rows(outputs: torch.Tensor):
        """logical (B,C,H,W) -> (tensor whose data pointer is the first NHWC row, pixel stride): a channels-last view -- the head's
        channel-padded buffer included -- is read in place, anything else is copied to NHWC once"""
        assert outputs.dim() == 4 and outputs.dtype == torch.float32
        b, c, h, w = outputs.shape
        st = outputs.stride()
        if (c == 1 or st[1] == 1) and st[3] >= c and st[2] == w * st[3] and (b == 1 or st[0] == h * st[2]):
            return outputs, st[3]
        return ops.to_nhwc(outputs), c

    def loss_and_grad(self, outputs: torch.Tensor, labels: torch.Tensor, scale: float = 1.0, max_valid: Optional[int] = None):
        """-> (loss vector (5,) [loss, lovasz, ce, n_valid, n_present], dlogits (B,H,W,pixel stride) = d(scale * loss)/d(logits) in the
        layout of the logits' NHWC buffer), both on the device (the training step's entry: no autograd, no readback)"""
        b, c, h, w = outputs.shape
        assert tuple(labels.shape) == (b, h, w), "labels must be (B, H, W)"
        rows, stride = self._rows(outputs)
        vec, dlogits, _ = seg_loss_nhwc(rows, stride, c, labels, self.ignore, scale, max_valid)
        return vec, dlogits.view(b, h, w, stride)

    def forward(self, outputs: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """outputs (B,C,H,W) logits, labels (B,H,W) integer -> the loss, a device scalar"""
        b, c, h, w = outputs.shape
        assert tuple(labels.shape) == (b, h, w), "labels must be (B, H, W)"
        rows, stride = self._rows(outputs)
        return seg_loss_nhwc(rows, stride, c, labels, self.ignore, want_grad=False)[0][0]


class SegHeadTrain:
    """SingleConvHead's training forward and explicit backward (kernel = 1), without autograd:
      logits = conv(x1; W[:, :C1]) + bias + bilinear_up(conv(x2; W[:, C1:]))
    ``weight`` / ``bias`` / ``grad_weight`` / ``grad_bias`` default to the head's parameters and fresh gradient tensors; the training
    step passes the views of its flat buffers.  ``side``: ops.SideStream for the weight-gradient launches.

    ``forward(x1, x2, vi=None)``: with ``vi`` (the iteration's VoxelIndex) x1 is a canvas of which only the pillars' cells are valid
    (the pillar-features first layer builds no dense canvas): the canvas part of the logits is then computed on the pillar rows and
    scattered, and the bias rides on the low-resolution term (interpolation weights sum to one)."""

    def __init__(self, head: "SingleConvHead", weight=None, bias=None, grad_weight=None, grad_bias=None, side=None):
        if head.conv.kernel_size != (1, 1):
            raise NotImplementedError("SegHeadTrain: only kernel=1 (the reference config) has a HIP path")
        self.head, self.n = head, head.num_classes
        self.npad = (self.n + 3) // 4 * 4
        self.w = head.conv.weight.detach() if weight is None else weight
        self.b = head.conv.bias.detach() if bias is None else bias
        hip.require_device(self.w, self.b)
        self.gw = torch.zeros_like(self.w) if grad_weight is None else grad_weight
        self.gb = torch.zeros_like(self.b) if grad_bias is None else grad_bias
        self.side = side
        self._plan = None
        self.x1 = self.x2 = self.vi = self.rows = self._d_rows = None

    def _layers(self, c1: int, rows: bool):
        """the packed layers of one form, refreshed from the current parameters; ``rows``: the bias rides on the low-resolution term"""
        n, npad, dev = self.n, self.npad, self.w.device
        p = self._plan
        if p is None or (p["c1"], p["rows"]) != (c1, rows):
            wa = torch.zeros((npad, c1, 1, 1), dtype=torch.float32, device=dev)
            wb = torch.zeros((npad, self.w.shape[1] - c1, 1, 1), dtype=torch.float32, device=dev)
            bias = torch.zeros((npad,), dtype=torch.float32, device=dev)
            p = self._plan = dict(c1=c1, rows=rows, wa=wa, wb=wb, bias=bias, a=ops.ConvLayer(wa, shift=None if rows else bias, act=ops.ACT_NONE),
                                  b=ops.ConvLayer(wb, shift=bias if rows else None, act=ops.ACT_NONE), da=ops.ConvDgrad(wa, 1, 0), db=ops.ConvDgrad(wb, 1, 0))
        p["wa"][:n].copy_(self.w[:, :c1])
        p["wb"][:n].copy_(self.w[:, c1:])
        p["bias"][:n].copy_(self.b)
        p["a"].repack(p["wa"], None if rows else p["bias"])
        p["b"].repack(p["wb"], p["bias"] if rows else None)
        p["da"].repack(p["wa"])
        p["db"].repack(p["wb"])
        return p

    def _dims(self, x1):
        return (C.c_int32 * 4)(x1.shape[0], 1, x1.shape[1], x1.shape[2])

    def forward(self, x1: torch.Tensor, x2: torch.Tensor, vi=None) -> torch.Tensor:
        """x1 (B,H,W,C1), x2 (B,h,w,C2) NHWC -> logits (B,H,W,npad) NHWC; keeps what backward needs"""
        hip.require_device(x1, x2)
        assert x1.shape[3] + x2.shape[3] == self.w.shape[1], "channel split does not match in_channels"
        p = self._layers(x1.shape[3], vi is not None)
        self.x1, self.x2, self.vi, self.rows, self._d_rows = x1, x2, vi, None, None
        st = hip.stream()
        if vi is None:
            out = p["a"](x1)
            low = p["b"](x2)
        else:
            b, h, w, c1 = x1.shape
            cap = max(vi.n_cap, 1)
            self.rows = torch.zeros((1, 1, cap, c1), dtype=torch.float32, device=x1.device)        # rows past the voxel count stay zero
            hip.call("pn_sparse_from_dense_nhwc", x1.data_ptr(), vi.unq_keys_ptr, cap, vi.num_voxels.data_ptr(), self._dims(x1), c1, self.rows.data_ptr(), st)
            row_logits = p["a"](self.rows)
            out = torch.empty((b, h, w, self.npad), dtype=torch.float32, device=x1.device)
            hip.call("pn_sparse_to_dense_nhwc", row_logits.data_ptr(), vi.unq_keys_ptr, cap, vi.num_voxels.data_ptr(), self._dims(x1), self.npad, out.data_ptr(), st)
            low = p["b"](x2)
        hip.call("pn_bilinear_upsample_add_f32", low.data_ptr(), low.shape[0], low.shape[1], low.shape[2], low.shape[3], out.shape[1], out.shape[2],
                 out.data_ptr(), st)
        return out

    def _on_side(self, fn, *reads):
        if self.side is not None:
            self.side.run(fn, *reads)
        else:
            fn()

    def backward_x2(self, dlogits: torch.Tensor, d_x2: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the low-resolution half: d(x2) (added into ``d_x2`` when given) and the gradients of W[:, C1:] and the bias"""
        p, n = self._plan, self.n
        d_low = bilinear_upsample_add_bwd(dlogits, self.x2.shape[1], self.x2.shape[2])
        x2, c1 = self.x2, p["c1"]

        def weight_grads():
            g = ops.conv_wgrad(x2, d_low, 1, 1, 1, 0, cout=n)
            self.gw[:, c1:].copy_(g)
            ops.channel_sum(dlogits, c=n, out=self.gb)

        self._on_side(weight_grads, d_low, x2, dlogits)
        return p["db"](d_low, out=d_x2, accumulate=d_x2 is not None)

    def _canvas_operands(self, dlogits: torch.Tensor):
        """(input, output gradient) of the canvas-half convolution: the dense maps, or after a forward with ``vi`` the pillar rows"""
        if self.vi is None:
            return self.x1, dlogits
        if self._d_rows is None:
            vi, cap = self.vi, max(self.vi.n_cap, 1)
            self._d_rows = torch.zeros((1, 1, cap, self.npad), dtype=torch.float32, device=dlogits.device)
            hip.call("pn_sparse_from_dense_nhwc", dlogits.data_ptr(), vi.unq_keys_ptr, cap, vi.num_voxels.data_ptr(), self._dims(self.x1), self.npad,
                     self._d_rows.data_ptr(), hip.stream())
        return self.rows, self._d_rows

    def backward_x1(self, dlogits: torch.Tensor, need_dx: bool = True):
        """the canvas half: the gradient of W[:, :C1] and (``need_dx``) d(x1) -- the dense (B,H,W,C1) canvas gradient, or, after a forward
        with ``vi``, the (n_cap, C1) pillar-feature gradient"""
        n, c1 = self.n, self._plan["c1"]
        x, d = self._canvas_operands(dlogits)

        def weight_grads():
            g = ops.conv_wgrad(x, d, 1, 1, 1, 0, cout=n)
            self.gw[:, :c1].copy_(g)

        self._on_side(weight_grads, d, x)
        if not need_dx:
            return None
        res = self._plan["da"](d)
        return res if self.vi is None else res.view(-1, c1)

    def backward_canvas(self, dlogits: torch.Tensor, d_x1: torch.Tensor) -> torch.Tensor:
        """d(x1) ADDED into ``d_x1``: a dense canvas gradient, or (forward with ``vi``) the (n_cap, C1) pillar-feature gradient"""
        x, d = self._canvas_operands(dlogits)
        self._plan["da"](d, out=d_x1.view(x.shape), accumulate=True)
        return d_x1

    def backward(self, dlogits: torch.Tensor):
        """-> (d_x1, d_x2); the parameter gradients land in ``gw`` / ``gb``"""
        d_x2 = self.backward_x2(dlogits)
        d_x1 = self.backward_x1(dlogits)
        if self.side is not None:
            self.side.join()
        return d_x1, d_x2


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
        """{'seg_loss': [weight * SegLoss(seg_preds, voxel_labels - 1)]} (seg_head.py:86-96); ``example['voxel_labels']``: (B,1,H,W)
        integer, 0 = unlabelled, on the device"""
        if self.loss_func is None:
            raise ValueError("SingleConvHead.loss: the head was built without a loss")
        seg_preds = preds_dicts["seg_preds"]
        seg_labels = get_labels(example["voxel_labels"].squeeze(1), tuple(seg_preds.shape[2:]))
        return {"seg_loss": [self.weight * self.loss_func(seg_preds, seg_labels)]}

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
            out.append({sample_token(example["metadata"], i): labels})
        return out

    @staticmethod
    def _flat_rows(example, dev, stacked=False):
        """device_only inputs: the grid indices of a sector -- or, ``stacked``, of PolarStreamBDCP's whole sweep -- as ONE (rows, 3) int64
        tensor (``example['valid_grid_ind']``: that tensor, or the per-sample list, concatenated on the device) and the samples' row
        offsets, device int32 (B + 1,): ``example['point_offsets']`` when present, otherwise built once from the host ``num_points`` and
        kept in the example (an upload: not capturable)"""
        gi = example["valid_grid_ind"]
        if not torch.is_tensor(gi):
            hip.require_device(*gi)
            gi = torch.cat([g.to(torch.int64) for g in gi], 0) if len(gi) > 1 else gi[0]
        hip.require_device(gi)
        gi = gi.to(torch.int64).contiguous()
        assert stacked or (gi.dim() == 2 and gi.shape[1] == 3), "valid_grid_ind must hold one [z, y, x] row per point"      # stacked: the caller's
        acc = None
        if example.get("point_offsets") is None:
            acc = prefix_sums(host_counts(example["num_points"]))
            assert stacked or acc[-1] <= gi.shape[0], "num_points does not match valid_grid_ind"
        offs = device_offsets(example, "point_offsets", acc, dev)
        well_formed = offs.dtype == torch.int32 and offs.dim() == 1 and offs.is_contiguous()
        if stacked:
            assert well_formed and offs.shape[0] == len(example["num_points"]) + 1, "point_offsets must be a contiguous int32 (nsectors * bs + 1,) tensor"
        else:
            assert well_formed, "point_offsets must be a contiguous int32 (B + 1,) tensor"
        return gi, offs

    @staticmethod
    def _device_list(det, bsz, wrong_type):
        """checks a device detection list of ``CenterHead.predict(device_only=True)`` under test_cfg.panoptic (TypeError ``wrong_type``
        when it is none) against the batch size -> the launch's box arguments (boxes, box stride, capacity, scores, labels, instance
        ids, counts)"""
        if not (isinstance(det, dict) and "instances" in det and "count" in det):
            raise TypeError(wrong_type)
        hip.require_device(*det.values())
        boxes = det["box3d_lidar"]
        cap = int(boxes.shape[1])
        assert boxes.dim() == 3 and boxes.shape[0] == bsz and boxes.dtype == torch.float32 and boxes.stride(2) == 1 and boxes.stride(0) == cap * boxes.stride(1)
        for k, dt in (("scores", torch.float32), ("label_preds", torch.int64), ("instances", torch.int64)):
            assert tuple(det[k].shape) == (bsz, cap) and det[k].dtype == dt and det[k].is_contiguous(), f"the device list's '{k}' must be a contiguous (B, cap) tensor"
        assert tuple(det["count"].shape) == (bsz,) and det["count"].dtype == torch.int32
        return (boxes.data_ptr(), boxes.stride(1), cap, det["scores"].data_ptr(), det["label_preds"].data_ptr(), det["instances"].data_ptr(),
                det["count"].data_ptr())

    @staticmethod
    def _sector_angle(test_cfg, voxel_shape, sec_id):
        """the rotation of sector ``sec_id``'s points into the sweep's frame: ``interval * sec_id``, cuboid: ``2 pi / interval * sec_id``
        (sector 0 reads no interval)"""
        if sec_id <= 0:
            return 0.0
        interval = float(test_cfg.get("interval") if hasattr(test_cfg, "get") else getattr(test_cfg, "interval"))
        return interval * sec_id if voxel_shape == "cylinder" else 2 * math.pi / interval * sec_id

    @staticmethod
    def _point_list(points, x_col):
        """the device point list with the Cartesian (x, y) in columns x_col, x_col + 1 -> (the list with unit inner stride, its row stride)"""
        hip.require_device(points)
        assert points.dim() == 2 and points.dtype == torch.float32 and points.shape[1] >= x_col + 2
        if points.numel() and points.stride(1) != 1:
            points = points.contiguous()
        return points, (points.stride(0) if points.shape[0] > 1 else points.shape[1])      # (the stride of a 0- or 1-row tensor is arbitrary)

    def _launch_batched(self, seg, gi, offs, labels, points=None, point_stride=0, x_col=0, angle=0.0, box_args=(None, 0, 0, None, None, None, None),
                        sem2box=None, score_thr=0.0, ins=None):
        """`pn_panoptic_points_batched_f32` on the (possibly channel-padded) NHWC logits, read in place; without points and
        ``box_args`` (``_device_list``): labels only"""
        bsz, ncls, h, w = seg.shape
        assert offs.shape[0] == bsz + 1, "point_offsets must have one entry per sample plus one"
        assert seg.stride(2) == w * seg.stride(3) and (bsz == 1 or seg.stride(0) >= h * w * seg.stride(3))
        hip.call("pn_panoptic_points_batched_f32", seg.data_ptr(), seg.stride(0) if bsz > 1 else 0, bsz, h, w, ncls, seg.stride(3), gi.data_ptr(),
                 offs.data_ptr(), gi.shape[0], hip.ptr(points), point_stride, x_col, math.cos(angle), math.sin(angle), *box_args, hip.ptr(sem2box),
                 float(score_thr), labels.data_ptr(), hip.ptr(ins), hip.stream())

    @torch.no_grad()
    def predict_panoptic_sweep(self, seg_preds, grid_ind, offsets, points, dets, test_cfg, *, voxel_shape, class_names, semantic2box=None,
                               score_thr=0.3, key_points_index=None, out_offsets=None, out_total=None, nsectors=1):
        """``predict_panoptic(device_only=True)`` for ALL sectors of a sweep in ONE launch (`pn_panoptic_points_sweep_f32`), for a detector
        that has every sector's logits and detection list at once (PolarStreamBDCP).  ``seg_preds``: the stacked (nsectors * bs, classes,
        H, W) channels-last logits, sector-major; ``grid_ind`` (rows, 3) int64 / ``offsets`` (nsectors * bs + 1,) int32: the flat rows of
        ``_flat_rows(example, dev, stacked=True)``; ``points`` (>= rows, F) the stacked point list, one row per ``grid_ind`` row; ``dets``: one
        device list of ``CenterHead.predict(device_only=True)`` under test_cfg.panoptic per sector (their capacities may differ), or None
        for the labels alone (``nsectors`` then says how the stacked batch splits, which matters to dataset order only).  Sector s is rotated by ``predict_panoptic``'s angle (``interval * s``; cuboid: ``2 pi / interval * s``),
        cos / sin taken as ``_launch_batched`` takes them, so the result is bit for bit that of one ``predict_panoptic`` per sector.
        -> (labels, ins): flat (rows,) int64 in stacked row order; ``ins`` is None without ``dets``.

        ``key_points_index`` (rows,) int64 on the device (the sectors' ``key_points_index`` in stacked row order) with ``out_offsets``
        (bs + 1,) int32 and ``out_total``: DATASET order (single_stage.py:118-128) -- the row of sample b lands at
        ``out_offsets[b] + key_points_index[row]`` of (out_total,) outputs, zero-filled first; rows pointing outside their sample are dropped.
        Nothing is read back and, once the class table is cached, nothing is uploaded."""
        hip.require_device(seg_preds, grid_ind, offsets)
        seg = seg_preds
        assert seg.dim() == 4 and seg.stride(1) == 1, "seg_preds must be the channels-last view produced by forward"
        total, ncls, h, w = seg.shape
        dev = seg.device
        nsec = int(nsectors) if dets is None else len(dets)      # the labels alone: any split of the stacked batch gives the same rows
        assert nsec >= 1 and total % nsec == 0, "the stacked batch is not a multiple of the number of sectors"
        bs = total // nsec
        assert grid_ind.dim() == 2 and grid_ind.shape[1] == 3 and grid_ind.dtype == torch.int64 and grid_ind.is_contiguous(), \
            "grid_ind must be a contiguous (rows, 3) int64 tensor"
        assert offsets.dtype == torch.int32 and offsets.dim() == 1 and offsets.is_contiguous() and offsets.shape[0] == total + 1, \
            "offsets must be a contiguous int32 (nsectors * bs + 1,) tensor"
        assert seg.stride(2) == w * seg.stride(3) and (total == 1 or seg.stride(0) >= h * w * seg.stride(3))
        rows = int(grid_ind.shape[0])
        dest = out_offs = None
        n_out = rows
        if key_points_index is not None:
            if out_offsets is None or out_total is None:
                raise ValueError("predict_panoptic_sweep: key_points_index needs out_offsets and out_total")
            hip.require_device(key_points_index, out_offsets)
            dest, out_offs, n_out = key_points_index, out_offsets, int(out_total)
            assert dest.dtype == torch.int64 and dest.dim() == 1 and dest.is_contiguous() and dest.shape[0] == rows, \
                "key_points_index must be a contiguous int64 tensor with one entry per grid_ind row"
            assert out_offs.dtype == torch.int32 and out_offs.dim() == 1 and out_offs.is_contiguous() and out_offs.shape[0] == bs + 1, \
                "out_offsets must be a contiguous int32 (bs + 1,) tensor"
        labels = torch.empty((n_out,), dtype=torch.int64, device=dev)
        points_ptr, point_stride, x_col, jobs, sem2box, ins = None, 0, 0, None, None, None      # the labels alone
        if dets is not None:
            sem2box = self._sem2box(class_names, semantic2box, ncls, dev)
            x_col = 3 if voxel_shape == "cylinder" else 0
            points, point_stride = self._point_list(points, x_col)
            assert rows <= points.shape[0], "valid_grid_ind has more rows than the point list: it must hold one row per point"
            points_ptr = points.data_ptr()
            jobs = (hip.PanopticSectorJob * nsec)()
            for s, det in enumerate(dets):
                j, angle = jobs[s], self._sector_angle(test_cfg, voxel_shape, s)
                j.boxes, j.box_stride, j.cap, j.scores, j.label_preds, j.instances, j.count = self._device_list(
                    det, bs, "predict_panoptic_sweep: every sector's list must be the device list of CenterHead.predict(device_only=True) under test_cfg.panoptic")
                j.cos_a, j.sin_a = math.cos(angle), math.sin(angle)
            ins = torch.empty((n_out,), dtype=torch.int64, device=dev)
        hip.call("pn_panoptic_points_sweep_f32", seg.data_ptr(), seg.stride(0) if total > 1 else 0, nsec, bs, h, w, ncls, seg.stride(3), grid_ind.data_ptr(),
                 offsets.data_ptr(), rows, points_ptr, point_stride, x_col, jobs, hip.ptr(sem2box), 0.0 if dets is None else float(score_thr), hip.ptr(dest),
                 hip.ptr(out_offs), n_out, labels.data_ptr(), hip.ptr(ins), hip.stream())
        return labels, ins

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
        angle = self._sector_angle(test_cfg, voxel_shape, int(sec_id))
        x_col = 3 if voxel_shape == "cylinder" else 0
        points, point_stride = self._point_list(example["points"], x_col)
        if device_only:
            box_args = self._device_list(ret_dict["det"], bsz, "predict_panoptic(device_only=True): ret_dict['det'] must be the device list of "
                                         "CenterHead.predict(device_only=True) under test_cfg.panoptic")
            gi, offs = self._flat_rows(example, dev)
            assert gi.shape[0] <= points.shape[0], "valid_grid_ind has more rows than the point list"
            labels = torch.empty((gi.shape[0],), dtype=torch.int64, device=dev)
            ins = torch.empty((gi.shape[0],), dtype=torch.int64, device=dev)
            self._launch_batched(seg, gi, offs, labels, points, point_stride, x_col, angle, box_args, sem2box, score_thr, ins)
            ret_dict["seg"], ret_dict["ins"] = labels, ins
            return ret_dict
        num = host_counts(example["num_points"])
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
            token = sample_token(example["metadata"], i)
            ret_dict["seg"].append({token: labels})
            ret_dict["ins"].append({token: ins})
        return ret_dict


class VoxelSegPreds:
    """``DeconvConvHead.forward_voxels``' result: ``logits`` (rows, NCpad) -- row r holds the ``num_classes`` logits of cell ``queries[r]``
    (an int32 key of ``level.dims``), rows at or beyond ``*count`` are undefined -- and the encoder's ``level`` (ops.SparseLevel) with the
    up-sampled neck map ``u``, which ``predict`` evaluates further cells from.  ``active``: the queries are the level's active set."""

    def __init__(self, logits, queries, count, level, u, active):
        self.logits, self.queries, self.count, self.level, self.u, self.active = logits, queries, count, level, u, active


@SEG_HEAD.register_module
class DeconvConvHead(SingleConvHead):
    """The 3-D segmentation head of the reference's VoxelNet seg configs (seg_head.py:223-264, ``height`` > 1):
    seg_preds = Conv2d((Cv + 1) D -> NC D, 3x3)(cat[conv1.dense(), deconv(x2)] viewed with the height folded into the channels), viewed as
    (B, NC, D, H, W).  Parameters as the reference's: ``deconv.weight`` (Cin, D, 2S, 2S), ``conv.weight`` (NC D, (Cv + 1) D, 3, 3),
    ``conv.bias``.

    The dense form is 3.2 TFLOP and a 1 GB logit tensor per sample at the config's shape, and its output is only read at cells that hold
    points: the head here evaluates the logits at a LIST of cells (csrc/voxel_seg.hip), by default the encoder's active set.  f32; the
    module itself is the eval-mode inference form, training runs on the tape at the labelled cells (train_voxel_seg.VoxelSegTrainStep)."""

    def __init__(self, kernel=3, num_classes=16, in_channels_voxel=16, in_channels=512, up_scale=8, weight=1, loss=None, height=1):
        # (the reference's ``kernel`` has no default; voxelnet_seg_10sweep.py leaves it out, which the reference cannot build -- 3 is the only form)
        if height == 1:
            raise NotImplementedError("DeconvConvHead: height == 1 (the 2-D form, deconvolution to in_channels // up_scale channels) is not built; "
                                      "the voxel-wise head needs height > 1")
        if height < 1:
            raise NotImplementedError(f"DeconvConvHead: height {height}")
        if kernel != 3:
            raise NotImplementedError(f"DeconvConvHead: kernel {kernel} is not built -- the voxel-wise logits kernel is the 3x3 form of the reference's configs")
        if in_channels_voxel != 16:
            raise NotImplementedError(f"DeconvConvHead: in_channels_voxel {in_channels_voxel} is not built -- the head reads the encoder's 16-channel conv1 level")
        if not 1 <= num_classes <= 32:
            raise NotImplementedError(f"DeconvConvHead: num_classes {num_classes} is not built (1..32 are)")
        if up_scale < 2 or up_scale % 2:
            raise NotImplementedError(f"DeconvConvHead: up_scale {up_scale} is not built -- the overlap-add kernel takes even scales")
        super().__init__(kernel, num_classes * height, height + in_channels_voxel * height, weight, loss)
        self.num_classes, self.height, self.up_scale, self.in_channels_voxel = num_classes, height, up_scale, in_channels_voxel
        self.deconv = nn.ConvTranspose2d(in_channels, height, kernel_size=2 * up_scale, stride=up_scale, padding=up_scale // 2, bias=False)

    def set_compute_dtype(self, dtype: str):
        if dtype != "f32":
            raise NotImplementedError("DeconvConvHead: bf16 is not built -- the voxel-wise head runs in f32 only")
        return self

    def _build_voxel_plan(self):
        w, b = self.conv.weight, self.conv.bias
        packed, pbias = ops.voxel_seg_pack(w, b, self.height, self.num_classes)
        return dict(deconv=ops.DeconvOverlap(self.deconv.weight, self.up_scale), packed=packed, bias=pbias)

    def _voxel_plan(self, *tensors):
        if any(t.dtype != torch.float32 for t in tensors):
            raise NotImplementedError("DeconvConvHead: bf16 is not built -- the voxel-wise head takes f32 tensors")
        eval_only(self, "DeconvConvHead")
        hip.require_device(*tensors)
        return self._plan.get(self, self._build_voxel_plan)

    def forward_nhwc(self, x1, x2):
        raise NotImplementedError("DeconvConvHead: there is no dense NHWC form -- forward_voxels(level0, x2_nhwc) evaluates the head at voxels")

    @torch.no_grad()
    def forward_voxels(self, level0, x2_nhwc: torch.Tensor, queries: Optional[torch.Tensor] = None, n_queries: Optional[torch.Tensor] = None) -> VoxelSegPreds:
        """level0: the encoder's ops.SparseLevel (``SpMiddleResNetFHD.forward_nhwc(..., return_conv1=True)``), x2_nhwc (B, h, w, Cin) the
        neck's output -> VoxelSegPreds with one logits row per query cell.  ``queries``: int32 keys ((b D + z) H + y) W + x, any cells in
        any order (``n_queries``: their device count; default all); default: the level's active set, in key order."""
        plan = self._voxel_plan(level0.feats, x2_nhwc)
        b, d, h, w = level0.dims
        if d != self.height:
            raise ValueError(f"DeconvConvHead: the level is {d} cells high, the head was built with height {self.height}")
        u = plan["deconv"](x2_nhwc)
        if tuple(u.shape) != (b, h, w, d):
            raise ValueError(f"DeconvConvHead: the up-sampled neck map is {tuple(u.shape[1:3])}, the voxel level {(h, w)} -- up_scale {self.up_scale} does not "
                             "match the encoder's down-sampling")
        active = queries is None
        if active:
            queries, n_queries = level0.keys, level0.count
        logits = ops.voxel_seg_logits(level0, u, plan["packed"], plan["bias"], self.num_classes, queries, n_queries)
        return VoxelSegPreds(logits, queries, n_queries, level0, u, active)

    @torch.no_grad()
    def forward(self, x1, x2):
        """logical dense tensors as the reference's signature (seg_head.py:251-264): x1 (B, 16, D, H, W) = ``conv1.dense()``, x2 (B, Cin, h, w)
        -> {'seg_preds': (B, NC, D, H, W)}.  The SMALL-SHAPE PARITY PATH: it builds the site index from the nonzero sites of x1 (a host
        read-back) and queries EVERY cell, which is the dense cost the voxel form exists to avoid; the detector uses ``forward_voxels``."""
        if x1.dim() != 5:
            raise NotImplementedError("DeconvConvHead: a 4-D x1 is the height == 1 form, which is not built")
        self._voxel_plan(x1, x2)
        level = ops.sparse_level_from_dense(x1)
        b, d, h, w = level.dims
        cells = torch.arange(b * d * h * w, dtype=torch.int32, device=x1.device)
        preds = self.forward_voxels(level, ops.to_nhwc(x2), cells)
        return {"seg_preds": preds.logits.view(b, d, h, w, -1)[..., :self.num_classes].permute(0, 4, 1, 2, 3)}

    def loss(self, example, preds_dicts, **kwargs):
        raise NotImplementedError("DeconvConvHead.loss: training the voxel segmentation head runs on the tape, at the labelled cells -- there are no dense "
                                  "seg_preds to take a loss from; use train_voxel_seg.VoxelSegTrainStep (or train_voxel_seg.voxel_seg_loss on a tape)")

    def predict_panoptic(self, *args, **kwargs):
        raise NotImplementedError("DeconvConvHead.predict_panoptic: panoptic fusion on voxel predictions is not built")

    def predict_panoptic_sweep(self, *args, **kwargs):
        raise NotImplementedError("DeconvConvHead.predict_panoptic_sweep: panoptic fusion on voxel predictions is not built")

    @torch.no_grad()
    def predict(self, example, preds_dicts, test_cfg=None, device_only=False, **kwargs):
        """per-point semantic labels (seg_head.py:170-192, the 5-D branch): 1 + argmax over the classes at every point's cell
        ``example['valid_grid_ind'][i]`` (n_i, 3) [z, y, x], ties to the lowest class.  ``preds_dicts``: ``forward_voxels``' result over the
        active set (or {'seg_preds': that}).  A point whose cell is no active site (hard voxelization dropped its voxel) gets the label of
        that cell's own logits, from a second launch over those cells; nothing is read back for it.
        -> list of {token: labels (n_i,) int64}, or with ``device_only`` the flat (rows,) int64 tensor in row order."""
        preds = preds_dicts["seg_preds"] if isinstance(preds_dicts, dict) else preds_dicts
        if not isinstance(preds, VoxelSegPreds) or not preds.active:
            raise TypeError("DeconvConvHead.predict takes the VoxelSegPreds of forward_voxels over the level's active set")
        plan = self._voxel_plan(preds.logits)
        lv = preds.level
        bsz = lv.dims[0]
        gi, offs, acc = self._point_rows(example, bsz, preds.logits.device)

        def miss_logits(keys, count):
            return ops.voxel_seg_logits(lv, preds.u, plan["packed"], plan["bias"], self.num_classes, keys, count)

        labels = ops.voxel_seg_point_labels(preds.logits, lv, self.num_classes, gi, offs, miss_logits)
        if device_only:
            return labels
        if acc is None:
            raise ValueError("DeconvConvHead.predict: per-sample lists need example['valid_grid_ind'] as a list; a flat tensor gives device_only=True")
        metas = example.get("metadata", list(range(bsz)))
        return [{sample_token(metas, i): labels[acc[i]:acc[i + 1]]} for i in range(bsz)]

    @staticmethod
    def _point_rows(example, bsz, dev):
        """``example['valid_grid_ind']`` -- the per-sample list of (n_i, 3) [z, y, x] device tensors, or ONE (rows, 3) tensor with
        ``example['point_offsets']`` (B + 1,) int32 on the device -> (rows int64, offsets, host prefix sums or None).  The counts come from
        the list itself: in a hard-voxel ``example`` ``num_points`` counts the points of a voxel, not of a sample."""
        gi = example["valid_grid_ind"]
        if torch.is_tensor(gi):
            offs = example.get("point_offsets")
            if offs is None:
                raise ValueError("DeconvConvHead.predict: a flat valid_grid_ind tensor needs example['point_offsets']")
            hip.require_device(gi, offs)
            assert offs.dtype == torch.int32 and offs.dim() == 1 and offs.is_contiguous() and offs.shape[0] == bsz + 1, \
                "point_offsets must be a contiguous int32 (B + 1,) tensor"
            return gi.to(torch.int64).contiguous(), offs, None
        assert len(gi) == bsz, "valid_grid_ind must hold one tensor per sample"
        hip.require_device(*gi)
        acc = prefix_sums([int(g.shape[0]) for g in gi])
        rows = torch.cat([g.to(torch.int64).view(-1, 3) for g in gi], 0).contiguous()
        return rows, torch.tensor(acc, dtype=torch.int32, device=dev), acc
