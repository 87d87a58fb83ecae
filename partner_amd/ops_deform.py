"""Deformable convolution (DCN v1, forward and backward) over the C ABI: ``DeformConvLayer``, the J-job launch of `pn_deform_conv3x3_f32`
(csrc/deform_conv.hip) behind the DCN CenterHead.  Replaces det3d/ops/dcn/deform_conv.py:16-60, 185-255 (DeformConvFunction.forward,
DeformConv) for the one shape the reference's models use: 3x3, stride 1, pad 1, dilation 1, groups 1, no bias, Cout = C."""
from __future__ import annotations

import ctypes
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
        self.packed_t, self._ws, self._bwd_stale = None, None, True      # the backward's transposed pack and workspace: made on first use
        self.repack(weights)

    def repack(self, weights: Sequence[torch.Tensor]) -> None:
        """pack new weights of the same shapes, on the current stream"""
        weights = [w.detach().contiguous() for w in weights]
        assert len(weights) == self.jobs and all(tuple(w.shape) == (self.c, self.c, 3, 3) and w.dtype == torch.float32 for w in weights)
        hip.require_device(*weights)
        self._src = weights      # (the pack launches are asynchronous: their sources stay referenced)
        self._bwd_stale = True
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

    # ------------------------------------------------------------------------------------------------------------ backward
    def prepack_bwd(self) -> None:
        """the transposed pack [job][tap][c][n] the data gradient reads, from the weights of the last ``repack``, on the current stream"""
        if self.packed_t is None:
            self.packed_t = _f32(self._floats * self.jobs, self.packed.device)
        st = hip.stream()
        for j, w in enumerate(self._src):
            hip.call("pn_deform_conv3x3_pack_bwd_f32", w.data_ptr(), self.c, self.packed_t.data_ptr() + 4 * self._floats * j, st)
        self._bwd_stale = False

    def _map(self, bhw, t, name, channels, channel_offset, aligned):
        """the rule every map of ``backward`` obeys: contiguous f32 NHWC of x's (B, H, W) that holds [channel_offset, + channels)"""
        hip.require_device(t)
        if t.dtype != torch.float32:
            raise NotImplementedError(f"DeformConvLayer.backward: only f32 maps are built (no bf16 deformable convolution); {name} is {t.dtype}")
        if t.dim() != 4 or not t.is_contiguous() or tuple(t.shape[:3]) != bhw:
            raise ValueError(f"DeformConvLayer.backward: {name} must be a contiguous NHWC map of x's (B, H, W) = {bhw}")
        if channel_offset < 0 or channel_offset + channels > t.shape[3]:
            raise ValueError(f"DeformConvLayer.backward: {name} needs {channels} channels from {channel_offset}, it has {t.shape[3]}")
        if aligned and (channel_offset % 4 != 0 or t.shape[3] % 4 != 0):
            raise ValueError(f"DeformConvLayer.backward: the channel offset {channel_offset} and the {t.shape[3]} channels of {name} must be "
                             "multiples of 4")

    def _saved(self, x, offset, out, dout, in_channel_offset, offset_channel_offset, out_channel_offset, dout_channel_offset):
        """checks the maps both halves of the backward read -> the leading arguments both C entries share after x, and (b, h, w)"""
        hip.require_device(x, offset)
        if x.dtype != torch.float32 or offset.dtype != torch.float32:
            raise NotImplementedError("DeformConvLayer.backward: only f32 maps are built (no bf16 deformable convolution)")
        if x.dim() != 4 or not x.is_contiguous():
            raise ValueError("DeformConvLayer.backward: x must be a contiguous NHWC map")
        bhw = tuple(x.shape[:3])
        self._map(bhw, x, "x", self.c, in_channel_offset, True)
        self._map(bhw, offset, "offset", self.offset_channels, offset_channel_offset, False)
        self._map(bhw, dout, "dout", self.out_channels, dout_channel_offset, True)
        if self.act == ACT_RELU and out is None:
            raise ValueError("DeformConvLayer.backward: act = ReLU needs the saved forward output `out` (its mask)")
        if out is not None:
            self._map(bhw, out, "out", self.out_channels, out_channel_offset, True)
        need = int(hip.load().pn_deform_conv3x3_bwd_workspace_bytes(*bhw, self.c, self.jobs))
        if need == 0:
            raise ValueError(f"DeformConvLayer.backward: a map of {bhw} pixels is past the kernels' 32-bit pixel indices")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        outp, outs = (out.data_ptr(), out.shape[3]) if out is not None else (None, 0)
        head = (x.data_ptr(), x.shape[3], in_channel_offset, offset.data_ptr(), offset.shape[3], offset_channel_offset)
        saved = (outp, outs, out_channel_offset, dout.data_ptr(), dout.shape[3], dout_channel_offset)
        return head, saved, bhw

    def backward(self, x: torch.Tensor, offset: torch.Tensor, out: Optional[torch.Tensor], dout: torch.Tensor, *,
                 d_x: Optional[torch.Tensor] = None, dx_channel_offset: int = 0, accumulate: bool = False,
                 d_offset: Optional[torch.Tensor] = None, doffset_channel_offset: int = 0,
                 d_weights: Optional[Sequence[torch.Tensor]] = None, wacc: bool = False, need_dx: bool = True,
                 in_channel_offset: int = 0, offset_channel_offset: int = 0, out_channel_offset: int = 0, dout_channel_offset: int = 0):
        """The gradients of ``__call__`` (csrc/deform_conv_bwd.hip).  x, offset and the channel offsets as in the forward call; ``out`` the
        saved forward output (its ReLU mask; may be None when act = ACT_NONE), read at ``out_channel_offset``; ``dout`` (B, H, W, >= J C) read
        at ``dout_channel_offset``.  -> (d_x, d_offset):
          d_x        the channels [dx_channel_offset, + C) of ``d_x`` ((B, H, W, C) when allocated here) are written, or added to when
                     ``accumulate``: the sum over the J jobs.  ``need_dx=False`` skips it (returns None).
          d_offset   the channels [doffset_channel_offset, + J dg 18) of ``d_offset``, in the offsets' order.
          d_weights  J tensors (C, C, 3, 3), written (``wacc``: added to); None leaves the weight gradient to a ``backward_weight`` call (a
                     training step queues that one on its side stream).
        The layer owns the workspace and reuses it; nothing is allocated once the shapes have been seen."""
        kw = dict(in_channel_offset=in_channel_offset, offset_channel_offset=offset_channel_offset, out_channel_offset=out_channel_offset,
                  dout_channel_offset=dout_channel_offset)
        head, saved, bhw = self._saved(x, offset, out, dout, **kw)
        if need_dx:
            if d_x is None:
                if accumulate:
                    raise ValueError("DeformConvLayer.backward: accumulate=True needs the d_x map to add to")
                d_x = torch.empty(bhw + (dx_channel_offset + self.c,), dtype=torch.float32, device=x.device)
            self._map(bhw, d_x, "d_x", self.c, dx_channel_offset, False)
        else:
            d_x = None
        if d_offset is None:
            d_offset = torch.empty(bhw + (doffset_channel_offset + self.offset_channels,), dtype=torch.float32, device=x.device)
        self._map(bhw, d_offset, "d_offset", self.offset_channels, doffset_channel_offset, False)
        if d_weights is not None:
            d_weights = self._weight_grads(d_weights)
        if self._bwd_stale:
            self.prepack_bwd()
        hip.call("pn_deform_conv3x3_bwd_data_f32", *head, self.packed_t.data_ptr(), *saved,
                 d_x.data_ptr() if d_x is not None else None, d_x.shape[3] if d_x is not None else 0, dx_channel_offset, int(bool(accumulate)),
                 d_offset.data_ptr(), d_offset.shape[3], doffset_channel_offset, *bhw, self.c, self.dg, self.jobs, self.act,
                 self._ws.data_ptr(), self._ws.numel(), hip.stream())
        if d_weights is not None:
            self.backward_weight(x, offset, out, dout, d_weights, wacc=wacc, **kw)
        return d_x, d_offset

    def _weight_grads(self, d_weights):
        d_weights = list(d_weights)
        if len(d_weights) != self.jobs or any(tuple(g.shape) != (self.c, self.c, 3, 3) or g.dtype != torch.float32 or not g.is_contiguous()
                                              for g in d_weights):
            raise ValueError(f"DeformConvLayer.backward: d_weights must be {self.jobs} contiguous f32 tensors ({self.c}, {self.c}, 3, 3)")
        hip.require_device(*d_weights)
        return d_weights

    def backward_weight(self, x: torch.Tensor, offset: torch.Tensor, out: Optional[torch.Tensor], dout: torch.Tensor,
                        d_weights: Sequence[torch.Tensor], *, wacc: bool = False, in_channel_offset: int = 0, offset_channel_offset: int = 0,
                        out_channel_offset: int = 0, dout_channel_offset: int = 0) -> None:
        """the weight gradients alone, on the current stream: ``d_weights[j]`` (C, C, 3, 3) of job j is written (``wacc``: added to).  It uses
        its own part of the workspace: it may run on another stream than ``backward`` of the same maps, at the same time."""
        head, saved, bhw = self._saved(x, offset, out, dout, in_channel_offset, offset_channel_offset, out_channel_offset, dout_channel_offset)
        d_weights = self._weight_grads(d_weights)
        ptrs = (ctypes.c_void_p * self.jobs)(*[g.data_ptr() for g in d_weights])      # (read by the entry before it returns)
        # the workspace was allocated on the stream of the first ``backward``; this call may run on another one (a step's side stream).
        # Recorded on it, a workspace that a larger shape replaces later is not handed out again while this launch still uses it.
        self._ws.record_stream(torch.cuda.current_stream())
        hip.call("pn_deform_conv3x3_bwd_weight_f32", *head, *saved, ctypes.addressof(ptrs), int(bool(wacc)), *bhw, self.c, self.dg, self.jobs,
                 self.act, self._ws.data_ptr(), self._ws.numel(), hip.stream())
