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
           "voxel_seg_point_labels", "voxel_seg_label_queries", "voxel_seg_query_index", "voxel_seg_unpack_grads", "voxel_seg_wgrad",
           "voxel_seg_dfeat", "voxel_seg_du", "deconv_overlap_bwd"]


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


# ------------------------------------------------------------------------------------------------------------------ training
def voxel_seg_label_queries(voxel_labels: torch.Tensor, num_classes: int, capacity: int):
    """the labelled cells of a DEVICE label map (B, D, H, W) or (B, 1, D, H, W), uint8 / int32 / int64, as a query list
    (seg_head.py:86-96: ``get_labels`` with equal shapes is ``labels - 1`` and 0 becomes the ignored -1)
    -> (keys (capacity,) int32 ascending, labels - 1 (capacity,) int32 with -1 behind the count, count (1,) int32, status (1,) int32:
    1 when more cells are labelled than ``capacity`` holds).  Labels outside [1, NC] are ignored.  Nothing is read back."""
    hip.require_device(voxel_labels)
    if voxel_labels.dim() == 5 and voxel_labels.shape[1] == 1:
        voxel_labels = voxel_labels[:, 0]
    assert voxel_labels.dim() == 4, "voxel_labels must be (B, D, H, W) or (B, 1, D, H, W)"
    kinds = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}
    if voxel_labels.dtype not in kinds:
        raise TypeError(f"voxel_seg_label_queries: labels of {voxel_labels.dtype} -- uint8, int32 and int64 are taken")
    lab = voxel_labels.contiguous()
    dims = [int(v) for v in lab.shape]
    dev, cap = lab.device, int(capacity)
    assert cap >= 1
    lib = hip.load()
    keys = torch.empty(cap, dtype=torch.int32, device=dev)
    out = torch.empty(cap, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = lib.pn_voxel_seg_label_queries_workspace_bytes(lab.numel())
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    hip.call("pn_voxel_seg_label_queries", lab.data_ptr(), kinds[lab.dtype], _dims(dims), int(num_classes), cap, keys.data_ptr(), out.data_ptr(),
             count.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, hip.stream())
    return keys, out, count, status


def voxel_seg_query_index(queries: torch.Tensor, n_dev: torch.Tensor, dims) -> torch.Tensor:
    """bitmap-rank index (``pn_sparse_index_from_coords``) over the cells of an ascending unique query list: the rank of a cell is its row.
    The keys are split into [b, z, y, x] rows with integer tensor operations (plumbing; the count stays on the device)."""
    hip.require_device(queries, n_dev)
    b, d, h, w = (int(v) for v in dims)
    n = int(queries.shape[0])
    assert n >= 1 and queries.dtype == torch.int32 and queries.is_contiguous(), "the query list holds at least one row of capacity"
    k = queries.to(torch.int64) & 0xFFFFFFFF
    coors = torch.stack([k // (d * h * w), (k // (h * w)) % d, (k // w) % h, k % w], 1).to(torch.int32).contiguous()
    dev = queries.device
    index = torch.empty(hip.load().pn_sparse_index_bytes(b * d * h * w), dtype=torch.uint8, device=dev)
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    hip.call("pn_sparse_index_from_coords", coors.data_ptr(), n, n_dev.data_ptr(), _dims(dims), index.data_ptr(), keys.data_ptr(), count.data_ptr(),
             rank.data_ptr(), hip.stream())
    return index


def voxel_seg_unpack_grads(d_packed: torch.Tensor, d_pbias: torch.Tensor, depth: int, num_classes: int):
    """the inverse of ``voxel_seg_pack`` on gradients: packed [z][slab][tap][16][NCpad] / [z][NCpad] -> the gradients of ``conv.weight``
    (NC D, 17 D, 3, 3) and ``conv.bias`` (NC D); tensor copies only"""
    d, nc = int(depth), int(num_classes)
    dh = (d + 15) // 16
    gp = d_packed.view(d, d + dh, 9, 16, -1)
    gw = torch.empty((nc, d, 17, d, 3, 3), dtype=torch.float32, device=gp.device)
    gw[:, :, :16] = gp[:, :d, :, :, :nc].reshape(d, d, 3, 3, 16, nc).permute(5, 0, 4, 1, 2, 3)
    gw[:, :, 16] = gp[:, d:, :, :, :nc].reshape(d, dh, 3, 3, 16, nc).permute(5, 0, 1, 4, 2, 3).reshape(nc, d, dh * 16, 3, 3)[:, :, :d]
    gb = d_pbias.view(d, -1)[:, :nc].t().reshape(nc * d)
    return gw.view(nc * d, 17 * d, 3, 3), gb.contiguous()


def _check_rows(dlogits, queries, num_classes):
    ncp = voxel_seg_class_pad(num_classes)
    assert queries.dtype == torch.int32 and queries.dim() == 1 and queries.is_contiguous()
    assert dlogits.dtype == torch.float32 and dlogits.is_contiguous() and tuple(dlogits.shape) == (int(queries.shape[0]), ncp), \
        "dlogits must hold one row of NCpad floats per query"
    return ncp


def voxel_seg_wgrad(level: SparseLevel, u: torch.Tensor, queries: torch.Tensor, n_dev: torch.Tensor, dlogits: torch.Tensor, num_classes: int):
    """-> (d packed weights, d packed bias) of ``voxel_seg_logits`` over an ASCENDING UNIQUE query list"""
    hip.require_device(level.feats, level.index, u, queries, n_dev, dlogits)
    b, d, h, w = level.dims
    ncp = _check_rows(dlogits, queries, num_classes)
    assert tuple(u.shape) == (b, h, w, d) and u.is_contiguous() and u.dtype == torch.float32
    assert level.feats.dtype == torch.float32 and level.feats.is_contiguous() and level.feats.shape[1] == 16
    dh = (d + 15) // 16
    d_packed = torch.empty((d, d + dh, 9, 16, ncp), dtype=torch.float32, device=u.device)
    d_pbias = torch.empty((d, ncp), dtype=torch.float32, device=u.device)
    if queries.shape[0] == 0:
        return d_packed.zero_(), d_pbias.zero_()
    hip.call("pn_voxel_seg_wgrad_f32", queries.data_ptr(), int(queries.shape[0]), n_dev.data_ptr(), dlogits.data_ptr(), _dims(level.dims),
             level.index.data_ptr(), level.feats.data_ptr(), u.data_ptr(), int(num_classes), d_packed.data_ptr(), d_pbias.data_ptr(), hip.stream())
    return d_packed, d_pbias


def voxel_seg_dfeat(level: SparseLevel, query_index: torch.Tensor, dlogits: torch.Tensor, packed_w: torch.Tensor, num_classes: int) -> torch.Tensor:
    """-> d_feats (rows of ``level.feats``, 16): the gradient of the level's conv1 features; rows at or beyond the level's count are zero"""
    hip.require_device(level.keys, level.count, query_index, dlogits, packed_w)
    ncp = voxel_seg_class_pad(num_classes)
    assert dlogits.dtype == torch.float32 and dlogits.is_contiguous() and dlogits.dim() == 2 and dlogits.shape[1] == ncp
    rows = int(level.feats.shape[0])
    assert level.keys.shape[0] >= rows
    out = torch.empty((rows, 16), dtype=torch.float32, device=dlogits.device)
    if dlogits.shape[0] == 0:
        return out.zero_()
    hip.call("pn_voxel_seg_dfeat_f32", level.keys.data_ptr(), rows, level.count.data_ptr(), _dims(level.dims), query_index.data_ptr(), int(dlogits.shape[0]),
             dlogits.data_ptr(), packed_w.data_ptr(), int(num_classes), out.data_ptr(), hip.stream())
    return out


def voxel_seg_du(dims, query_index: torch.Tensor, dlogits: torch.Tensor, packed_w: torch.Tensor, num_classes: int) -> torch.Tensor:
    """-> d_u (B, H, W, D): the gradient of the up-sampled map, every element written"""
    hip.require_device(query_index, dlogits, packed_w)
    ncp = voxel_seg_class_pad(num_classes)
    assert dlogits.dtype == torch.float32 and dlogits.is_contiguous() and dlogits.dim() == 2 and dlogits.shape[1] == ncp
    b, d, h, w = (int(v) for v in dims)
    out = torch.empty((b, h, w, d), dtype=torch.float32, device=dlogits.device)
    if dlogits.shape[0] == 0:
        return out.zero_()
    hip.call("pn_voxel_seg_du_f32", _dims(dims), query_index.data_ptr(), int(dlogits.shape[0]), dlogits.data_ptr(), packed_w.data_ptr(), int(num_classes),
             out.data_ptr(), hip.stream())
    return out


def deconv_overlap_bwd(d_u: torch.Tensor, up_scale: int) -> torch.Tensor:
    """d_u (B, h S, w S, D) -> d_cols (B h w, 2S 2S D): the adjoint of ``pn_deconv_overlap_f32``"""
    hip.require_device(d_u)
    s = int(up_scale)
    assert d_u.dim() == 4 and d_u.is_contiguous() and d_u.dtype == torch.float32 and d_u.shape[1] % s == 0 and d_u.shape[2] % s == 0
    b, hh, ww, d = d_u.shape
    h, w = hh // s, ww // s
    out = torch.empty((b * h * w, 4 * s * s * d), dtype=torch.float32, device=d_u.device)
    hip.call("pn_deconv_overlap_bwd_f32", d_u.data_ptr(), b, h, w, s, d, out.data_ptr(), hip.stream())
    return out
