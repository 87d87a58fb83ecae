"""Deformable convolution (DCN v1, forward) over the C ABI: ``DeformConvLayer``, the J-job launch of `pn_deform_conv3x3_f32`
(csrc/deform_conv.hip) behind the DCN CenterHead.  Replaces det3d/ops/dcn/deform_conv.py:16-60, 185-255 (DeformConvFunction.forward,
DeformConv) for the one shape the reference's models use: 3x3, stride 1, pad 1, dilation 1, groups 1, no bias, Cout = C."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import hip
from .hip import ACT_NONE, ACT_RELU
from .ops_common import _f32

__all__ = ["DeformConvLayer"]


class DeformConvLayer:
    """J deformable 3x3 convolutions C -> C that read ONE input map and one wide offset map and write channel slices of one output map, in
    one launch.

    weights: J tensors (Cout, C, 3, 3) in torch layout (``DeformConv.weight``), Cout = C in {32, 64, 128}; ``dg`` deformable groups with
    C / dg a multiple of 4; ``act``: ACT_NONE | ACT_RELU.  Everything else is refused with a ValueError that names the rule; DCN v2
    (modulated), bias, strides, dilation and convolution groups are not built (nothing in the reference's models uses them).
    The packed copy [job][tap][n][c] is made here, on the current stream; ``repack`` refreshes it from new weights of the same shape (a module
    that owns a layer rebuilds it through its ``PlanCache`` whenever its parameters change, as it does its ``ConvLayer``s)."""

    def __init__(self, weights: Sequence[torch.Tensor], dg: int = 1, act: int = ACT_NONE):
        weights = list(weights)
        if not weights:
            raise ValueError("DeformConvLayer: at least one weight (job) is needed")
        for w in weights:
            if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
                raise ValueError(f"DeformConvLayer: weights must be (Cout, C, 3, 3) -- only the 3x3 kernel is built; got {tuple(w.shape)}")
            if w.shape[0] != w.shape[1]:
                raise ValueError(f"DeformConvLayer: Cout must equal C (got Cout = {w.shape[0]}, C = {w.shape[1]})")
            if w.shape != weights[0].shape:
                raise ValueError("DeformConvLayer: every job's weight must have the same shape")
        c, dg = int(weights[0].shape[1]), int(dg)
        if c not in (32, 64, 128):
            raise ValueError(f"DeformConvLayer: C must be 32, 64 or 128 (got C = {c})")
        if dg < 1 or c % dg != 0 or (c // dg) % 4 != 0:
            raise ValueError(f"DeformConvLayer: C / dg must be a multiple of 4 (got C = {c}, dg = {dg})")
        if act not in (ACT_NONE, ACT_RELU):
            raise ValueError("DeformConvLayer: act must be ACT_NONE or ACT_RELU")
        if any(w.dtype != torch.float32 for w in weights):
            raise NotImplementedError("DeformConvLayer: only f32 is built (no bf16 deformable convolution)")
        hip.require_device(*weights)
        self.c, self.dg, self.act, self.jobs = c, dg, int(act), len(weights)
        self.offset_channels = self.jobs * dg * 18
        self.out_channels = self.jobs * c
        self._floats = int(hip.load().pn_deform_conv3x3_packed_weight_floats(c))
        self.packed = _f32(self._floats * self.jobs, weights[0].device)
        self.repack(weights)

    def repack(self, weights: Sequence[torch.Tensor]) -> None:
        """pack new weights of the same shapes, on the current stream"""
        weights = [w.detach().contiguous() for w in weights]
        assert len(weights) == self.jobs and all(tuple(w.shape) == (self.c, self.c, 3, 3) and w.dtype == torch.float32 for w in weights)
        hip.require_device(*weights)
        self._src = weights      # (the pack launches are asynchronous: their sources stay referenced)
        st = hip.stream()
        for j, w in enumerate(weights):
            hip.call("pn_deform_conv3x3_pack_f32", w.data_ptr(), self.c, self.packed.data_ptr() + 4 * self._floats * j, st)

    def __call__(self, x: torch.Tensor, offset: torch.Tensor, out: Optional[torch.Tensor] = None, in_channel_offset: int = 0,
                 offset_channel_offset: int = 0, out_channel_offset: int = 0) -> torch.Tensor:
        """x: NHWC (B, H, W, Cx), read at channels [in_channel_offset, + C); offset: (B, H, W, >= J dg 18), job j's channels
        [offset_channel_offset + 18 dg j, + 18 dg) in the reference's order (group, tap, (dh, dw)); writes the channels
        [out_channel_offset + C j, + C) of ``out`` ((B, H, W, J C) when allocated here)."""
        hip.require_device(x, offset)
        if x.dtype != torch.float32 or offset.dtype != torch.float32:
            raise NotImplementedError("DeformConvLayer: only f32 maps are built (no bf16 deformable convolution)")
        if x.dim() != 4 or not x.is_contiguous() or offset.dim() != 4 or not offset.is_contiguous() or offset.shape[:3] != x.shape[:3]:
            raise ValueError("DeformConvLayer: x and offset must be contiguous NHWC maps of the same (B, H, W)")
        b, h, w, cx = x.shape
        if in_channel_offset % 4 != 0 or cx % 4 != 0 or in_channel_offset < 0 or in_channel_offset + self.c > cx:
            raise ValueError(f"DeformConvLayer: the input slice [{in_channel_offset}, +{self.c}) must fit the map's {cx} channels, both multiples of 4")
        if offset_channel_offset < 0 or offset_channel_offset + self.offset_channels > offset.shape[3]:
            raise ValueError(f"DeformConvLayer: the offset map needs J * dg * 18 = {self.offset_channels} channels from {offset_channel_offset}, "
                             f"it has {offset.shape[3]}")
        if out is None:
            out = torch.empty((b, h, w, out_channel_offset + self.out_channels), dtype=torch.float32, device=x.device)
        hip.require_device(out)
        if (out.dim() != 4 or not out.is_contiguous() or out.dtype != torch.float32 or out.shape[:3] != x.shape[:3] or out_channel_offset < 0
                or out_channel_offset + self.out_channels > out.shape[3]):
            raise ValueError(f"DeformConvLayer: out must be a contiguous f32 (B, H, W, >= {out_channel_offset + self.out_channels}) map")
        hip.call("pn_deform_conv3x3_f32", x.data_ptr(), cx, in_channel_offset, offset.data_ptr(), offset.shape[3], offset_channel_offset,
                 self.packed.data_ptr(), out.data_ptr(), out.shape[3], out_channel_offset, b, h, w, self.c, self.dg, self.jobs, self.act,
                 hip.stream())
        return out
