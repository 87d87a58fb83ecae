"""Voxel-wise segmentation over the C ABI (csrc/voxel_seg.hip): the transposed convolution of ``UpsampleShelhamer`` as one GEMM plus an
overlap-add, the logits of DeconvConvHead (height > 1) at a list of cells, and the per-point labels.  Replaces
det3d/models/seg_heads/seg_head.py:195-264 (and ``predict``, :170-192, on its 3-D branch) for f32 inference."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import torch

from . import hip
from .ops_token import GemmLayer

__all__ = ["SparseLevel", "DeconvOverlap", "sparse_level_from_dense", "voxel_seg_class_pad", "voxel_seg_pack", "voxel_seg_logits",
           "voxel_seg_point_labels"]


@dataclass
class SparseLevel:
    """one resolution level of the sparse encoder: ``feats`` (cap, C) in key order (rows at or beyond ``count`` are undefined), the
    bitmap-rank ``index`` buffer, the active ``keys`` (cap,) int32 of ``dims`` = [B, D, H, W] in ascending order, the device ``count``"""
    feats: torch.Tensor
    index: torch.Tensor
    keys: torch.Tensor
    count: torch.Tensor
    cap: int
    dims: List[int]


def _dims(dims):
    return (C.c_int32 * 4)(*[int(v) for v in dims])


def sparse_level_from_dense(x1: torch.Tensor) -> SparseLevel:
    """logical dense (B, C, D, H, W) -> the level of its nonzero sites (a site is active where any channel is nonzero).  Reads the site
    count back: the small-shape parity path, not the frame's."""
    hip.require_device(x1)
    b, c, d, h, w = x1.shape
    dev = x1.device
    dims = [b, d, h, w]
    coors = (x1 != 0).any(1).nonzero().to(torch.int32).contiguous()
    v = max(int(coors.shape[0]), 1)
    if coors.shape[0] == 0:
        coors = torch.full((1, 4), -1, dtype=torch.int32, device=dev)      # no site: one row outside the grid, which the index ignores
    lib = hip.load()
    index = torch.empty(lib.pn_sparse_index_bytes(b * d * h * w), dtype=torch.uint8, device=dev)
    keys = torch.empty(v, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    rank = torch.empty(v, dtype=torch.int32, device=dev)
    n_dev = torch.full((1,), v, dtype=torch.int32, device=dev)
    st = hip.stream()
    hip.call("pn_sparse_index_from_coords", coors.data_ptr(), v, n_dev.data_ptr(), _dims(dims), index.data_ptr(), keys.data_ptr(), count.data_ptr(),
             rank.data_ptr(), st)
    cl = coors.long().clamp_(min=0)
    rows = x1.float()[cl[:, 0], :, cl[:, 1], cl[:, 2], cl[:, 3]].contiguous()
    feats = torch.zeros((v, c), dtype=torch.float32, device=dev)
    hip.call("pn_sparse_permute_rows", rows.data_ptr(), rank.data_ptr(), v, n_dev.data_ptr(), c, feats.data_ptr(), st)
    return SparseLevel(feats=feats, index=index, keys=keys, count=count, cap=v, dims=dims)


class DeconvOverlap:
    """``ConvTranspose2d(Cin -> D, kernel 2S, stride S, padding S/2, bias=False)`` (UpsampleShelhamer, seg_head.py:195-212) on NHWC maps:
    one GEMM (B h w, Cin) x (Cin, 2S 2S D) on the token-GEMM kernel, then `pn_deconv_overlap_f32` adds the at most four column entries of
    every output element.  weight: (Cin, D, 2S, 2S), torch layout."""

    def __init__(self, weight: torch.Tensor, up_scale: int):
        s = int(up_scale)
        if s < 2 or s % 2:
            raise NotImplementedError(f"DeconvOverlap: up_scale {up_scale} -- the overlap-add kernel takes even scales")
        cin, d, kh, kw = weight.shape
        assert (kh, kw) == (2 * s, 2 * s), "the transposed convolution's kernel must be 2 * up_scale"
        if cin % 4:
            raise NotImplementedError(f"DeconvOverlap: {cin} input channels -- the GEMM takes multiples of 4")
        self.s, self.d, self.cin = s, int(d), int(cin)
        self.gemm = GemmLayer(weight.detach().float().permute(2, 3, 1, 0).reshape(4 * s * s * d, cin).contiguous())      # row (ky 2S + kx) D + c

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """x (B, h, w, Cin) NHWC -> (B, h S, w S, D) NHWC"""
        hip.require_device(x)
        assert x.dim() == 4 and x.dtype == torch.float32 and x.shape[3] == self.cin
        b, h, w, _ = x.shape
        cols = self.gemm(x.contiguous().view(b * h * w, self.cin))
        out = torch.empty((b, h * self.s, w * self.s, self.d), dtype=torch.float32, device=x.device)
        hip.call("pn_deconv_overlap_f32", cols.data_ptr(), b, h, w, self.s, self.d, out.data_ptr(), hip.stream())
        return out


def voxel_seg_class_pad(num_classes: int) -> int:
    """the padded class count of a logits row (0: that many classes are not built)"""
    return int(hip.load().pn_voxel_seg_class_pad(int(num_classes)))


def voxel_seg_pack(weight: torch.Tensor, bias: torch.Tensor, depth: int, num_classes: int):
    """``conv.weight`` (NC D, 17 D, 3, 3) / ``conv.bias`` (NC D) of DeconvConvHead -> (packed weights [z][D slabs z' | ceil(D / 16) slabs of
    u][tap][16][NCpad], packed bias [z][NCpad]), zero padded; a layout change only, done once per plan with tensor copies"""
    d, nc = int(depth), int(num_classes)
    ncp = voxel_seg_class_pad(nc)
    if ncp == 0:
        raise NotImplementedError(f"voxel_seg_pack: {nc} classes -- 1..32 are built")
    assert tuple(weight.shape) == (nc * d, 17 * d, 3, 3) and tuple(bias.shape) == (nc * d,)
    w = weight.detach().float().view(nc, d, 17, d, 3, 3)                      # [c, z, k, z', ky, kx]
    dh = (d + 15) // 16
    packed = torch.zeros((d, d + dh, 9, 16, ncp), dtype=torch.float32, device=w.device)
    packed[:, :d, :, :, :nc] = w[:, :, :16].permute(1, 3, 4, 5, 2, 0).reshape(d, d, 9, 16, nc)
    wu = torch.zeros((nc, d, dh * 16, 3, 3), dtype=torch.float32, device=w.device)
    wu[:, :, :d] = w[:, :, 16]                                                 # [c, z, h, ky, kx]
    packed[:, d:, :, :, :nc] = wu.view(nc, d, dh, 16, 3, 3).permute(1, 2, 4, 5, 3, 0).reshape(d, dh, 9, 16, nc)
    assert packed.numel() == hip.load().pn_voxel_seg_packed_weight_floats(d, nc)
    pb = torch.zeros((d, ncp), dtype=torch.float32, device=w.device)
    pb[:, :nc] = bias.detach().float().view(nc, d).t()
    return packed.contiguous(), pb.contiguous()


def voxel_seg_logits(level: SparseLevel, u: torch.Tensor, packed_w: torch.Tensor, packed_b: torch.Tensor, num_classes: int,
                     queries: Optional[torch.Tensor] = None, n_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> (n_cap, NCpad) logits of the cells ``queries`` (int32 keys of ``level.dims``; default: the level's active set, its count on the
    device); rows at or beyond ``*n_dev`` are not written (``out``: a buffer to write into)"""
    hip.require_device(level.feats, level.index, u, packed_w, packed_b)
    b, d, h, w = level.dims
    assert level.feats.dtype == torch.float32 and level.feats.is_contiguous() and level.feats.shape[1] == 16, "the level's features must be (rows, 16) f32"
    assert tuple(u.shape) == (b, h, w, d) and u.is_contiguous() and u.dtype == torch.float32, "u must be the (B, H, W, D) NHWC up-sampled map"
    ncp = voxel_seg_class_pad(num_classes)
    assert tuple(packed_w.shape[:1]) == (d,) and packed_w.numel() == hip.load().pn_voxel_seg_packed_weight_floats(d, num_classes)
    if queries is None:
        queries, n_dev = level.keys, level.count
    hip.require_device(queries)
    assert queries.dtype == torch.int32 and queries.dim() == 1 and queries.is_contiguous()
    n_cap = int(queries.shape[0])
    if out is None:
        out = torch.empty((n_cap, ncp), dtype=torch.float32, device=u.device)
    assert tuple(out.shape) == (n_cap, ncp) and out.is_contiguous() and out.dtype == torch.float32
    if n_cap == 0:
        return out
    if n_dev is None:
        n_dev = torch.full((1,), n_cap, dtype=torch.int32, device=u.device)
    hip.call("pn_voxel_seg_logits_f32", queries.data_ptr(), n_cap, n_dev.data_ptr(), _dims(level.dims), level.index.data_ptr(), level.feats.data_ptr(),
             u.data_ptr(), packed_w.data_ptr(), packed_b.data_ptr(), int(num_classes), out.data_ptr(), hip.stream())
    return out


def voxel_seg_point_labels(rows: torch.Tensor, level: SparseLevel, num_classes: int, grid_ind: torch.Tensor, offsets: torch.Tensor, miss_logits=None):
    """labels (n,) int64 = 1 + argmax of the row of every point's cell; ``rows``: the logits of the level's active set in key order.
    ``miss_logits(keys, count) -> rows``: evaluates the cells of points that lie in no active site (a second logits launch); without it
    those points get 0.  Nothing is read back."""
    hip.require_device(rows, grid_ind, offsets)
    assert grid_ind.dtype == torch.int64 and grid_ind.dim() == 2 and grid_ind.shape[1] == 3 and grid_ind.is_contiguous()
    assert offsets.dtype == torch.int32 and offsets.is_contiguous() and offsets.shape[0] == level.dims[0] + 1
    n, dev = int(grid_ind.shape[0]), rows.device
    labels = torch.empty((n,), dtype=torch.int64, device=dev)
    mk = mr = mc = None
    if miss_logits is not None and n:
        mk, mr = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        mc = torch.empty(1, dtype=torch.int32, device=dev)
    st = hip.stream()
    hip.call("pn_voxel_seg_point_labels", rows.data_ptr(), int(num_classes), level.index.data_ptr(), _dims(level.dims), grid_ind.data_ptr() if n else None,
             offsets.data_ptr(), n, labels.data_ptr(), hip.ptr(mk), hip.ptr(mr), hip.ptr(mc), st)
    if mk is not None:
        extra = miss_logits(mk, mc)
        hip.call("pn_voxel_seg_scatter_labels", extra.data_ptr(), int(num_classes), mr.data_ptr(), n, mc.data_ptr(), n, labels.data_ptr(), st)
    return labels
