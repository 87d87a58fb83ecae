"""CPU ORACLE -- TEST INFRASTRUCTURE ONLY.  NOT the product, never shipped, never timed as
"our" number.  Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s
``cpu_baseline`` leg may import this module; ``partner_amd`` must not.

A CPU restatement of the reference's polar-voxel encode -> BEV backbone -> centre head
path, written functionally over a ``state_dict`` (name -> tensor) instead of as
``nn.Module``s.  Integer / index stages are numpy (and mirrored in plain C in
``polar_voxel.c``); floating-point network stages use torch CPU fp32 functional ops.

Parity pin: every function here is checked by ``tests/test_oracle_golden.py`` against the
fixtures in ``tests/golden/*.npz`` that ``tests/golden/make_golden.py`` captured by running
the reference itself (imported from /root/reference) on the same deterministic inputs.
The reference ships no tests of its own, so those captures are the only pin.
Third-party arithmetic restated here without an upstream pin: ``torch_scatter``
(scatter_mean / scatter_max semantics; unpinned in the reference).

Reference locations are cited per function as file:line under /root/reference.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

Tensor = torch.Tensor
SD = Dict[str, Tensor]


# ======================================================================================
# V0  cart -> polar decoration            det3d/datasets/pipelines/utils.py:34-47
# ======================================================================================
def cart_to_polar(pc: np.ndarray) -> np.ndarray:
    """[x,y,z,rest...] -> [rho,phi,z,x,y,rest...] (cylinder branch), dtype preserved."""
    x, y = pc[:, 0], pc[:, 1]
    rho = np.sqrt(x * x + y * y)
    phi = np.arctan2(y, x)
    out = np.empty((pc.shape[0], pc.shape[1] + 2), dtype=pc.dtype)
    out[:, 0], out[:, 1], out[:, 2] = rho, phi, pc[:, 2]
    out[:, 3], out[:, 4] = x, y
    out[:, 5:] = pc[:, 3:]
    return out


# ======================================================================================
# V1  dynamic voxelization indices        det3d/datasets/pipelines/voxelization.py:165-168
#     grid size                           det3d/core/input/voxel_generator.py:6-17
#     batch index prepend                 det3d/torchie/parallel/collate.py:157-164
# ======================================================================================
def grid_size_of(pc_range: Sequence[float], voxel_size: Sequence[float]) -> np.ndarray:
    r = np.asarray(pc_range, dtype=np.float32)
    v = np.asarray(voxel_size, dtype=np.float32)
    return np.round((r[3:] - r[:3]) / v).astype(np.int64)


def grid_index(points: np.ndarray, pc_range, voxel_size, grid_size=None) -> np.ndarray:
    """(N,>=3) fp32 polar points -> (N,3) int64 [z, theta, r]; out-of-range points are clamped.

    fp32 subtract, fp32 true divide, clip to [0, G-1], floor -- in that order.
    """
    lo = np.asarray(pc_range, dtype=np.float32)[:3]
    vs = np.asarray(voxel_size, dtype=np.float32)
    g = grid_size_of(pc_range, voxel_size) if grid_size is None else np.asarray(grid_size, np.int64)
    q = (points[:, :3].astype(np.float32) - lo) / vs  # fp32
    q = np.minimum(np.maximum(q.astype(np.float64), 0.0), (g - 1).astype(np.float64))
    return np.floor(q).astype(np.int64)[:, ::-1].copy()


def with_batch_index(per_sample: List[np.ndarray]) -> np.ndarray:
    return np.concatenate([np.concatenate([np.full((g.shape[0], 1), b, g.dtype), g], 1)
                           for b, g in enumerate(per_sample)], 0)


# ======================================================================================
# unique rows in lexicographic order      torch.unique(dim=0) at
#                                         det3d/models/readers/pillar_encoder.py:398
# ======================================================================================
def linear_key(grid_ind: np.ndarray, grid_size) -> np.ndarray:
    """(N,4) [b,z,theta,r] -> int64 key ((b*Z+z)*T+theta)*R+r  (grid_size = [R,T,Z])."""
    R, T, Z = (int(v) for v in grid_size[:3])
    g = grid_ind.astype(np.int64)
    return ((g[:, 0] * Z + g[:, 1]) * T + g[:, 2]) * R + g[:, 3]


def unique_voxels(grid_ind: np.ndarray, grid_size) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> unq (V,4) int64 lexicographically sorted, unq_inv (N,) int64, unq_cnt (V,) int64."""
    R, T, Z = (int(v) for v in grid_size[:3])
    key = linear_key(grid_ind, grid_size)
    uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    unq = np.empty((uk.shape[0], 4), np.int64)
    unq[:, 3] = uk % R
    unq[:, 2] = (uk // R) % T
    unq[:, 1] = (uk // (R * T)) % Z
    unq[:, 0] = uk // (R * T * Z)
    return unq, inv.astype(np.int64).reshape(-1), cnt.astype(np.int64)


# ======================================================================================
# torch_scatter semantics (third-party, unpinned): segment mean / max over unq_inv
#   call sites  pillar_encoder.py:66,236 ; voxel_encoder.py:43
# ======================================================================================
def scatter_mean(x: Tensor, inv: Tensor, n: int) -> Tensor:
    acc = torch.zeros((n, x.shape[1]), dtype=x.dtype)
    acc.index_add_(0, inv, x)
    cnt = torch.bincount(inv, minlength=n).clamp_(min=1).to(x.dtype)
    return acc / cnt[:, None]


def scatter_max(x: Tensor, inv: Tensor, n: int) -> Tensor:
    out = torch.full((n, x.shape[1]), float("-inf"), dtype=x.dtype)
    return out.scatter_reduce(0, inv[:, None].expand_as(x), x, reduce="amax", include_self=True)


# ======================================================================================
# V3  DynamicVoxelEncoderV1               det3d/models/readers/voxel_encoder.py:38-45
#     VoxelFeatureExtractorV3             det3d/models/readers/voxel_encoder.py:15-22
# ======================================================================================
def dynamic_voxel_mean(points: np.ndarray, grid_ind: np.ndarray, grid_size):
    unq, inv, _ = unique_voxels(grid_ind, grid_size)
    f = scatter_mean(torch.from_numpy(points), torch.from_numpy(inv), unq.shape[0])
    return f.numpy(), unq


def hard_voxel_mean(voxels: np.ndarray, num_points: np.ndarray) -> np.ndarray:
    v = torch.from_numpy(voxels)
    return (v.sum(dim=1) / torch.from_numpy(num_points).to(v.dtype).view(-1, 1)).numpy()


# ======================================================================================
# V2  hard voxelization                   det3d/ops/point_cloud/point_cloud_ops.py:7-72,146-224
# ======================================================================================
def hard_voxelize(points: np.ndarray, voxel_size, pc_range, max_points: int, max_voxels: int):
    """First-come voxel ids in point order, <=max_points kept per voxel, <=max_voxels voxels;
    out-of-range points dropped (a voxel that already exists keeps accepting points after the
    voxel budget is exhausted).  -> voxels (V,P,F) f32, coors (V,3) int32 [z,theta,r], num (V,) int32
    """
    vs = np.asarray(voxel_size, dtype=points.dtype)
    rg = np.asarray(pc_range, dtype=points.dtype)
    grid = np.round((rg[3:] - rg[:3]) / vs).astype(np.int32)
    c = np.floor((points[:, :3] - rg[:3]) / vs)  # same dtype arithmetic as the reference loop
    ok = np.all((c >= 0) & (c < grid), axis=1)
    ci = c[ok].astype(np.int64)[:, ::-1]  # z, theta, r
    pidx = np.nonzero(ok)[0]
    key = (ci[:, 0] * int(grid[1]) + ci[:, 1]) * int(grid[0]) + ci[:, 2]
    uk, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")  # voxel id = rank of first appearance
    rank_of = np.empty_like(order)
    rank_of[order] = np.arange(order.shape[0])
    vid = rank_of[inv.reshape(-1)]
    nv = min(int(uk.shape[0]), int(max_voxels))
    keep = vid < nv
    vid, pidx, ci = vid[keep], pidx[keep], ci[keep]
    # slot of each point inside its voxel = number of earlier points of the same voxel
    so = np.argsort(vid, kind="stable")
    vs_sorted = vid[so]
    start = np.searchsorted(vs_sorted, np.arange(nv), side="left")
    slot = np.empty_like(vid)
    slot[so] = np.arange(vid.shape[0]) - start[vs_sorted]
    counts = np.bincount(vid, minlength=nv)
    voxels = np.zeros((nv, max_points, points.shape[1]), points.dtype)
    sel = slot < max_points
    voxels[vid[sel], slot[sel]] = points[pidx[sel]]
    coors = np.zeros((nv, 3), np.int32)
    coors[vid] = ci  # every point of a voxel carries the same coordinate
    num = np.minimum(counts, max_points).astype(np.int32)
    return voxels, coors, num


# ======================================================================================
# V4  DynamicPFNet                        det3d/models/readers/pillar_encoder.py:338-406,63-71,228-249
# ======================================================================================
def pfn_feature_deco(points: Tensor, inv: Tensor, grid_ind: Tensor, n_vox: int, voxel_size, pc_range,
                     voxel_shape="cylinder", xyz_cluster=True, raz_cluster=True, xy_center=True,
                     ra_center=True) -> Tensor:
    vx, vy = voxel_size[0], voxel_size[1]
    x_off, y_off = vx / 2 + pc_range[0], vy / 2 + pc_range[1]
    dt = points.dtype
    cols = [points]
    c1 = grid_ind[:, 3:4].to(dt) * vx + x_off
    c2 = grid_ind[:, 2:3].to(dt) * vy + y_off
    if xyz_cluster or xy_center:
        xyz = points[:, :3] if voxel_shape == "cuboid" else points[:, [3, 4, 2]]
        if xyz_cluster:
            cols.append(xyz - scatter_mean(xyz, inv, n_vox)[inv])
        if xy_center:
            if voxel_shape == "cuboid":
                xc, yc = c1, c2
            else:
                xc, yc = c1 * torch.cos(c2), c1 * torch.sin(c2)
            cols += [xyz[:, 0:1] - xc, xyz[:, 1:2] - yc]
    if raz_cluster or ra_center:
        ra = points[:, :2] if voxel_shape != "cuboid" else points[:, -2:]
        if raz_cluster:
            src = ra if xyz_cluster else torch.cat([ra, points[:, 2:3]], 1)
            cols.append(src - scatter_mean(src, inv, n_vox)[inv])
        if ra_center:
            if voxel_shape == "cuboid":
                rc, ac = torch.sqrt(c1 ** 2 + c2 ** 2), torch.atan2(c2, c1)
            else:
                rc, ac = c1, c2
            cols += [ra[:, 0:1] - rc, ra[:, 1:2] - ac]
    return torch.cat(cols, dim=1)


def dynamic_pfn(sd: SD, prefix: str, points: np.ndarray, grid_ind: np.ndarray, grid_size, voxel_size, pc_range,
                **deco_kw) -> Tuple[Tensor, np.ndarray, np.ndarray]:
    """-> features (V,C_last), unq (V,4) int64, unq_inv (N,).  BN layers exist in the
    state_dict but are NOT applied on the dynamic path (pillar_encoder.py:63-71)."""
    unq, inv_np, _ = unique_voxels(grid_ind, grid_size)
    V = unq.shape[0]
    inv = torch.from_numpy(inv_np)
    x = pfn_feature_deco(torch.from_numpy(points), inv, torch.from_numpy(grid_ind.astype(np.int64)), V, voxel_size,
                         pc_range, **deco_kw)
    n_layers = len([k for k in sd if k.startswith(prefix + "pfn_layers.") and k.endswith("linear.weight")])
    for i in range(n_layers):
        w = sd[f"{prefix}pfn_layers.{i}.linear.weight"]
        x = F.relu(x @ w.t())
        xm = scatter_max(x, inv, V)
        x = xm if i == n_layers - 1 else torch.cat([x, xm[inv]], dim=1)
    return x, unq, inv_np


# ======================================================================================
# V5  DynamicPPScatter                    det3d/models/readers/pillar_encoder.py:418-432
# ======================================================================================
def scatter_canvas(feats: Tensor, unq: np.ndarray, batch: int, grid_size) -> Tensor:
    nx, ny = int(grid_size[0]), int(grid_size[1])
    canvas = torch.zeros((batch, feats.shape[1], ny, nx), dtype=feats.dtype)
    u = torch.from_numpy(unq.astype(np.int64))
    canvas[u[:, 0], :, u[:, 2], u[:, 3]] = feats
    return canvas


# ======================================================================================
# B1  RPN                                 det3d/models/necks/rpn.py:23-159
# ======================================================================================
def _bn(sd: SD, p: str, x: Tensor, training: bool, eps=1e-3, momentum=0.01) -> Tensor:
    return F.batch_norm(x, None if training else sd[p + "running_mean"], None if training else sd[p + "running_var"],
                        sd[p + "weight"], sd[p + "bias"], training=training, momentum=momentum, eps=eps)


def rpn(sd: SD, prefix: str, x: Tensor, layer_nums, ds_layer_strides, ds_num_filters, us_layer_strides,
        us_num_filters, training=False, return_all=False, **_ignored):
    """Blocks: ZeroPad(1)+conv3x3(stride s)+BN+ReLU then k x [conv3x3 pad1 + BN + ReLU];
    deblock i: ConvTranspose2d(k=s,s) if us>1 else Conv2d(k=round(1/us), stride same); concat."""
    start = len(layer_nums) - len(us_layer_strides)
    ups, blocks = [], []
    for i, n in enumerate(layer_nums):
        bp = f"{prefix}blocks.{i}."
        x = F.conv2d(F.pad(x, (1, 1, 1, 1)), sd[bp + "1.weight"], stride=int(ds_layer_strides[i]))
        x = F.relu(_bn(sd, bp + "2.", x, training))
        for j in range(n):
            x = F.conv2d(x, sd[f"{bp}{4 + 3 * j}.weight"], padding=1)
            x = F.relu(_bn(sd, f"{bp}{5 + 3 * j}.", x, training))
        blocks.append(x)
        if i - start >= 0:
            us = us_layer_strides[i - start]
            dp = f"{prefix}deblocks.{i - start}."
            if us > 1:
                y = F.conv_transpose2d(x, sd[dp + "0.weight"], stride=int(us))
            else:
                k = int(np.round(1 / us))
                y = F.conv2d(x, sd[dp + "0.weight"], stride=k)
            ups.append(F.relu(_bn(sd, dp + "1.", y, training)))
    out = torch.cat(ups, dim=1) if ups else x
    return (out, blocks, ups) if return_all else out


# ======================================================================================
# H2  CenterHeadSingle / CenterHeadSinglePos   det3d/models/bbox_heads/center_head_parallel.py:27-59,70-196,199-284
#     RSNorm                                   det3d/models/utils/norm.py:58-75
# ======================================================================================
def rs_norm(x: Tensor, w: Tensor, b: Tensor, num_heads: int, num_groups: int, eps=1e-5) -> Tensor:
    """Range-stratified GroupNorm: split the last (range) axis into ``num_groups`` strata,
    stack them on channels, GroupNorm(num_heads*num_groups groups), un-stack."""
    parts = x.chunk(num_groups, dim=-1)
    y = F.group_norm(torch.cat(parts, 1), num_heads * num_groups, w, b, eps)
    return torch.cat(y.chunk(num_groups, dim=1), dim=-1)


def range_stratified(sd: SD, p: str, x: Tensor, kernel=(3, 3), nheads=1, ngroups=8) -> Tensor:
    """Per-range-stratum 3x3 conv (groups=ngroups*nheads, own weights per stratum) + GroupNorm + ReLU.
    Azimuth is zero-padded; each stratum sees one halo column of its range neighbours (zeros at the ends)."""
    pa, pr = kernel[0] // 2, kernel[1] // 2
    x = F.pad(x, (0, 0, pa, pa))
    step = x.shape[-1] // ngroups
    if pr > 0:
        x = F.pad(x, (pr, pr, 0, 0))
        x = torch.cat([x[:, :, :, step * i: step * (i + 1) + 2 * pr] for i in range(ngroups)], 1)
    else:
        x = torch.cat([x[:, :, :, step * i: step * (i + 1)] for i in range(ngroups)], 1)
    x = F.conv2d(x, sd[p + "conv.0.weight"], sd[p + "conv.0.bias"], groups=ngroups * nheads)
    x = F.relu(F.group_norm(x, ngroups * nheads, sd[p + "conv.1.weight"], sd[p + "conv.1.bias"], 1e-5))
    return torch.cat(x.chunk(ngroups, dim=1), dim=-1)


def polar_pos_encoding(voxel_generator: dict, out_size_factor: int) -> Tensor:
    """(1,5,A,R) [r cos, r sin, r, cos, sin] at cell corners (center_head_parallel.py:229-260)."""
    pr, vs, ns = list(voxel_generator["range"]), voxel_generator["voxel_size"], voxel_generator["nsectors"]
    min_az, max_az = pr[1], pr[4]
    ref4 = min_az + (max_az - min_az) / ns
    r_size = round((pr[3] - pr[0]) / vs[0] / out_size_factor)
    a_size = round((ref4 - pr[1]) / vs[1] / out_size_factor)
    ga, gr = torch.meshgrid(torch.arange(a_size), torch.arange(r_size), indexing="ij")
    ga = ga * out_size_factor * vs[1] + pr[1]
    gr = gr * out_size_factor * vs[0] + pr[0]
    c, s = torch.cos(ga), torch.sin(ga)
    return torch.stack([gr * c, gr * s, gr, c, s])[None]


def _head_branch(sd: SD, p: str, x: Tensor, name: str, num_conv: int) -> Tensor:
    """One merged head: 'reg' -> RangeStratified + 1x1; 'a_b' -> grouped convs; else plain convs."""
    if "reg" in name:
        y = range_stratified(sd, f"{p}{name}.0.", x)
        return F.conv2d(y, sd[f"{p}{name}.1.weight"], sd[f"{p}{name}.1.bias"])
    groups = len(name.split("_")) if "_" in name else 1
    y, idx = x, 0
    for _ in range(num_conv - 1):
        y = F.conv2d(y, sd[f"{p}{name}.{idx}.weight"], sd[f"{p}{name}.{idx}.bias"], padding=1, groups=groups)
        ch = y.shape[1]
        y = F.relu(F.group_norm(y, ch, sd[f"{p}{name}.{idx + 1}.weight"], sd[f"{p}{name}.{idx + 1}.bias"], 1e-5))
        idx += 3
    return F.conv2d(y, sd[f"{p}{name}.{idx}.weight"], sd[f"{p}{name}.{idx}.bias"], padding=1, groups=groups)


def center_head_single(sd: SD, prefix: str, x: Tensor, common_heads: dict, num_hm_conv=2, pos_encoding=None,
                       return_internals=False):
    """CenterHeadSingle.forward; with ``pos_encoding`` also the position-conditioned
    calibration of CenterHeadSinglePos (hm input = x*W(pos)+b(pos))."""
    p = prefix
    xs = F.conv2d(x, sd[p + "shared_conv.0.weight"], sd[p + "shared_conv.0.bias"], padding=1)
    xs = F.relu(rs_norm(xs, sd[p + "shared_conv.1.groupnorm.weight"], sd[p + "shared_conv.1.groupnorm.bias"], 1, 4))
    heads = dict(common_heads)
    heads["hm"] = (None, num_hm_conv)
    cal_w = cal_b = None
    x_hm = xs
    if pos_encoding is not None:
        cw = torch.tanh(F.conv2d(pos_encoding, sd[p + "calibration_weight.0.weight"], sd[p + "calibration_weight.0.bias"], padding=1))
        cal_w = torch.tanh(F.conv2d(cw, sd[p + "calibration_weight.2.weight"], sd[p + "calibration_weight.2.bias"]))
        cb = torch.tanh(F.conv2d(pos_encoding, sd[p + "calibration_bias.0.weight"], sd[p + "calibration_bias.0.bias"], padding=1))
        cal_b = F.conv2d(cb, sd[p + "calibration_bias.2.weight"], sd[p + "calibration_bias.2.bias"])
        x_hm = xs * cal_w + cal_b
    ret = {}
    for name, (_, num_conv) in heads.items():
        out = _head_branch(sd, p, x_hm if name == "hm" else xs, name, num_conv)
        if "_" in name:
            for j, (nm, t) in enumerate(zip(name.split("_"), out.chunk(len(name.split("_")), dim=1))):
                ret[nm] = t
        else:
            ret[name] = out
    if return_internals:
        return ret, dict(shared=xs, cal_weight=cal_w, cal_bias=cal_b)
    return ret


# ======================================================================================
# H1  CenterHead / SepHead                det3d/models/bbox_heads/center_head.py:65-109,166-242
# ======================================================================================
def center_head(sd: SD, prefix: str, x: Tensor, tasks_num_classes: Sequence[int], common_heads: dict,
                num_hm_conv=2) -> List[Dict[str, Tensor]]:
    xs = F.relu(F.conv2d(x, sd[prefix + "shared_conv.0.weight"], sd[prefix + "shared_conv.0.bias"], padding=1))
    rets = []
    for t, ncls in enumerate(tasks_num_classes):
        heads = dict(common_heads)
        heads["hm"] = (ncls, num_hm_conv)
        d = {}
        for name, (_, num_conv) in heads.items():
            y, idx = xs, 0
            for _ in range(num_conv - 1):
                kp = f"{prefix}tasks.{t}.{name}.{idx}."
                y = F.relu(F.conv2d(y, sd[kp + "weight"], sd[kp + "bias"], padding=1))
                idx += 2
            kp = f"{prefix}tasks.{t}.{name}.{idx}."
            d[name] = F.conv2d(y, sd[kp + "weight"], sd[kp + "bias"], padding=1)
        rets.append(d)
    return rets


def single_conv_head(sd: SD, prefix: str, x1: Tensor, x2: Tensor) -> Tensor:
    """SingleConvHead.forward (det3d/models/seg_heads/seg_head.py:75-83): bilinear up-sampling of the RPN output to the canvas,
    concatenation, one convolution.  -> seg_preds (B, num_classes, H, W)"""
    x = F.interpolate(x2, size=x1.shape[-2:], mode="bilinear")
    w = sd[prefix + "conv.weight"]
    return F.conv2d(torch.cat([x1, x], dim=1), w, sd[prefix + "conv.bias"], padding=w.shape[-1] // 2)


def seg_point_labels(seg_preds: Tensor, valid_grid_ind: Sequence[np.ndarray]) -> List[np.ndarray]:
    """SingleConvHead.predict (seg_head.py:176-195) for a 2-D prediction map: label = 1 + argmax at [theta, r] of every point"""
    lab = torch.argmax(seg_preds, dim=1) + 1
    return [lab[i][torch.from_numpy(np.asarray(g))[:, 1], torch.from_numpy(np.asarray(g))[:, 2]].numpy() for i, g in enumerate(valid_grid_ind)]


# ======================================================================================
# L1  CenterHead.loss                     det3d/models/bbox_heads/center_head.py:244-288
#     FastFocalLoss / RegLoss             det3d/models/losses/centernet_loss.py:26-54,6-24
# ======================================================================================
def _gather_at(feat: Tensor, ind: Tensor) -> Tensor:
    b, c, h, w = feat.shape
    flat = feat.permute(0, 2, 3, 1).reshape(b, h * w, c)
    return flat.gather(1, ind[:, :, None].expand(-1, -1, c))


def center_loss(preds: Dict[str, Tensor], hm_t: Tensor, ind: Tensor, mask: Tensor, cat: Tensor, anno_box: Tensor,
                code_weights: Sequence[float], weight: float):
    hm = torch.clamp(torch.sigmoid(preds["hm"]), min=1e-4, max=1 - 1e-4)
    m = mask.to(hm.dtype)  # mask.float() for float32 predictions; float64 ones keep num_pos + 1e-4 in float64
    neg = (torch.log(1 - hm) * hm ** 2 * (1 - hm_t) ** 4).sum()
    pos_pred = _gather_at(hm, ind).gather(2, cat[:, :, None])
    pos = (torch.log(pos_pred) * (1 - pos_pred) ** 2 * m[:, :, None]).sum()
    num_pos = m.sum()
    hm_loss = -neg if num_pos == 0 else -(pos + neg) / num_pos
    if "vel" in preds:
        box = torch.cat((preds["reg"], preds["height"], preds["dim"], preds["vel"], preds["rot"]), 1)
        tgt = anno_box
    else:
        box = torch.cat((preds["reg"], preds["height"], preds["dim"], preds["rot"]), 1)
        tgt = anno_box[..., [0, 1, 2, 3, 4, 5, -2, -1]]
    pred = _gather_at(box, ind)
    l1 = (pred * m[:, :, None] - tgt * m[:, :, None]).abs() / (m.sum() + 1e-4)
    box_loss = l1.sum(dim=(0, 1))
    loc = (box_loss * box_loss.new_tensor(list(code_weights))).sum()
    return dict(det_loss=hm_loss + weight * loc, hm_loss=hm_loss, loc_loss=loc, loc_loss_elem=box_loss, num_positive=num_pos)


# ======================================================================================
# A1  SetBlock (global representation re-alignment)   det3d/models/utils/set_transformer.py:56-493
#     bev_pos                                         det3d/models/detectors/voxelnet.py:10-25
# ======================================================================================
def waymo_bev_pos(x_size=144, y_size=256, pc_range=(0.3, -3.14368, -2.0, 75.18, 3.14368, 4.0),
                  voxel_size=(0.065, 0.00307, 0.15), scale=8) -> Tensor:
    """(1, x_size(r), y_size(theta), 4) = [x, y, r, phi] at BEV cell centres."""
    ri = torch.linspace(0, x_size - 1, x_size)[:, None].expand(x_size, y_size) + 0.5
    ti = torch.linspace(0, y_size - 1, y_size)[None, :].expand(x_size, y_size) + 0.5
    r = ri * voxel_size[0] * scale + pc_range[0]
    phi = ti * voxel_size[1] * scale + pc_range[1]
    return torch.stack([r * torch.cos(phi), r * torch.sin(phi), r, phi], dim=2)[None]


def _lin(sd: SD, p: str, x: Tensor) -> Tensor:
    return F.linear(x, sd[p + "weight"], sd.get(p + "bias"))


def _mlp(sd: SD, p: str, x: Tensor) -> Tensor:
    return _lin(sd, p + "fc2.", F.gelu(_lin(sd, p + "fc1.", x)))


def _ln(sd: SD, p: str, x: Tensor) -> Tensor:
    return F.layer_norm(x, (x.shape[-1],), sd[p + "weight"], sd[p + "bias"], 1e-5)


def _pos_bias(sd: SD, p: str, rel: Tensor, train=False) -> Tensor:
    """rel (G,2,L) -> (G,heads,L): Conv1d(2->16) + BN1d + ReLU + Conv1d(16->heads); BN1d with the running statistics, or
    (train: module.train() semantics) the batch statistics -- the running buffers are left untouched."""
    y = F.conv1d(rel, sd[p + "0.weight"], sd[p + "0.bias"])
    if train:
        y = F.batch_norm(y, None, None, sd[p + "1.weight"], sd[p + "1.bias"], True, 0.1, 1e-5)
    else:
        y = F.batch_norm(y, sd[p + "1.running_mean"], sd[p + "1.running_var"], sd[p + "1.weight"], sd[p + "1.bias"], False, 0.1, 1e-5)
    return F.conv1d(F.relu(y), sd[p + "3.weight"], sd[p + "3.bias"])


def _cols(t: Tensor, B: int, H: int, W: int, heads: int) -> Tensor:
    """(B, H*W, C) tokens -> per theta-column windows (B*W, heads, H, C/heads)."""
    C = t.shape[-1]
    return t.view(B, H, W, heads, C // heads).permute(0, 2, 3, 1, 4).reshape(B * W, heads, H, C // heads)


def _raw_view_keypoints(t: Tensor, B: int, K: int, W: int, heads: int) -> Tensor:
    """The reference reinterprets the (B, K*W, C) key-point buffer as (B, C, K, W) WITHOUT a
    transpose (set_transformer.py:331-334,417-425); reproduce that literally.
    -> (B*W, heads, K, C/heads)"""
    C = t.shape[-1]
    q = t.reshape(B, C, K, W).view(B, heads, C // heads, K, W)
    return q.permute(0, 4, 1, 3, 2).reshape(B * W, heads, K, C // heads)


def set_attention(sd: SD, p: str, x: Tensor, pos_cart: Tensor, reso, heads: int, K=4, win_w=8, shift=False,
                  return_topidx=False, top_override=None, return_scores=False, train=False):
    """SetAttention.forward for H_sp=H (full range column), W_sp=1.  x (B,L,C); pos_cart (B,H,W,2).
    train: BatchNorm1d of the position MLPs in training mode (dropout / drop-path rates are taken as 0)."""
    H, W = reso
    B, L, C = x.shape
    hd = C // heads
    scale = hd ** -0.5
    shortcut = x
    xn = _ln(sd, p + "norm1.", x).view(B, H, W, C)
    xpos = pos_cart
    sh = win_w // 2 if shift else 0
    if sh:
        xn = torch.roll(xn, -sh, 2)
        xpos = torch.roll(xpos, -sh, 2)
    # key-point selection: per theta-column, top-K strict-ish local maxima of the channel mean along range
    s = xn.mean(dim=3)  # (B,H,W)
    st = s.permute(0, 2, 1)
    lm = torch.zeros_like(st)
    lm[:, :, 1:-1] = F.max_pool1d(st, 3, 1, 0)
    s = (st * (lm == st)).permute(0, 2, 1)
    scores = s
    top = s.argsort(dim=1, descending=True)[:, :K, :]  # (B,K,W)
    if top_override is not None:
        # checker option: use externally supplied key-point rows.  torch's argsort is not stable, so when
        # fewer than K positive local maxima exist the reference's choice among the tied zeros is
        # implementation defined (it differs between torch's CPU and GPU sorts); the HIP kernel breaks
        # ties towards the smaller row index.
        top = top_override
    kp = xn.gather(1, top[..., None].expand(-1, -1, -1, C)).reshape(B, K * W, C)
    kpos = xpos.gather(1, top[..., None].expand(-1, -1, -1, 2))  # (B,K,W,2)
    xt = xn.reshape(B, L, C)
    # per-column position tensors (G=B*W, 2, n)
    xp = xpos.permute(0, 2, 3, 1).reshape(B * W, 2, H)
    sp = kpos.permute(0, 2, 3, 1).reshape(B * W, 2, K)

    # ---- sector attention 1: key points <- their column ------------------------------------
    q = "sector_attn1."
    rel = (sp[:, :, :, None] - xp[:, :, None, :]).reshape(B * W, 2, K * H)
    bias = _pos_bias(sd, p + q + "pos_embedding_cart.", rel, train).view(B * W, heads, K, H)
    qq = _raw_view_keypoints(_lin(sd, p + q + "proj_q.", kp), B, K, W, heads) * scale
    kk = _cols(_lin(sd, p + q + "proj_k.", xt), B, H, W, heads)
    vv = _cols(_lin(sd, p + q + "proj_v.", xt), B, H, W, heads)
    a = torch.softmax(qq @ kk.transpose(-2, -1) + bias, dim=-1)
    o = (a @ vv).transpose(1, 2).reshape(B, W, K, C).permute(0, 2, 1, 3).reshape(B, K * W, C)
    s1 = kp + _lin(sd, p + q + "proj.", o)
    s1 = s1 + _mlp(sd, p + q + "mlp.", _ln(sd, p + q + "norm2.", s1))

    # ---- range attention among key points, windows K x win_w -------------------------------
    q = "range_attn."
    nw = W // win_w
    n = K * win_w
    sn = _ln(sd, p + q + "norm1.", s1)
    wp = kpos.view(B, 1, K, nw, win_w, 2).permute(0, 1, 3, 5, 2, 4).reshape(B * nw, 2, n)
    rel = (wp[:, :, :, None] - wp[:, :, None, :]).reshape(B * nw, 2, n * n)
    bias = _pos_bias(sd, p + q + "pos_embedding_cart.", rel, train).view(B * nw, heads, n, n)

    def win(t):
        return t.view(B, K, nw, win_w, heads, hd).permute(0, 2, 4, 1, 3, 5).reshape(B * nw, heads, n, hd)

    qq = win(_lin(sd, p + q + "proj_q.", sn)) * scale
    kk = win(_lin(sd, p + q + "proj_k.", sn))
    vv = win(_lin(sd, p + q + "proj_v.", sn))
    a = torch.softmax(qq @ kk.transpose(-2, -1) + bias, dim=-1)
    o = (a @ vv).transpose(1, 2).reshape(B, nw, K, win_w, C).permute(0, 2, 1, 3, 4).reshape(B, K * W, C)
    s2 = s1 + _lin(sd, p + q + "proj.", o)
    s2 = s2 + _mlp(sd, p + q + "mlp.", _ln(sd, p + q + "norm2.", s2))

    # ---- sector attention 2: column <- key points (no proj / mlp inside) --------------------
    q = "sector_attn2."
    rel = (xp[:, :, :, None] - sp[:, :, None, :]).reshape(B * W, 2, H * K)
    bias = _pos_bias(sd, p + q + "pos_embedding_cart.", rel, train).view(B * W, heads, H, K)
    qq = _cols(_lin(sd, p + q + "proj_q.", xt), B, H, W, heads) * scale
    kk = _raw_view_keypoints(_lin(sd, p + q + "proj_k.", s2), B, K, W, heads)
    vv = _raw_view_keypoints(_lin(sd, p + q + "proj_v.", s2), B, K, W, heads)
    a = torch.softmax(qq @ kk.transpose(-2, -1) + bias, dim=-1)
    o = (a @ vv).transpose(1, 2).reshape(B, W, H, C).permute(0, 2, 1, 3)  # (B,H,W,C)
    if sh:
        o = torch.roll(o, sh, 2)
    o = o.reshape(B, L, C)
    y = shortcut + _lin(sd, p + "proj.", o)
    y = y + _mlp(sd, p + "mlp.", _ln(sd, p + "norm2.", y))
    if return_scores:
        return y, top, scores
    return (y, top) if return_topidx else y


def set_block(sd: SD, prefix: str, x: Tensor, pos: Tensor, reso, heads=4, K=4, win_w=8, shift=False) -> Tensor:
    """SetBlock.forward with embed_dim_scale == 1 (the only configuration VoxelNetV3 builds)."""
    B = x.shape[0]
    return set_attention(sd, prefix + "attns.", x, pos[..., :2].repeat(B, 1, 1, 1), reso, heads, K, win_w, shift)


# ======================================================================================
# D1  PointPillars (dynamic branch) end-to-end      det3d/models/detectors/point_pillars.py:40-110
# ======================================================================================
def pointpillars_forward(sd: SD, cfg: dict, points: np.ndarray, grid_ind: np.ndarray, batch: int,
                         return_stages=False):
    """cfg: the model dict of the config (reader / neck / bbox_head sub-dicts, reference schema)."""
    rd, nk, hd = cfg["reader"], cfg["neck"], cfg["bbox_head"]
    vg = hd["voxel_generator"]
    gsz = grid_size_of(vg["range"], vg["voxel_size"])
    feats, unq, inv = dynamic_pfn(sd, "reader.", points, grid_ind, gsz, rd["voxel_size"], rd["pc_range"],
                                  voxel_shape=rd.get("voxel_shape", "cylinder"), xyz_cluster=rd["xyz_cluster"],
                                  raz_cluster=rd["raz_cluster"], xy_center=rd["xy_center"], ra_center=rd["ra_center"])
    x1 = scatter_canvas(feats, unq, batch, gsz)
    x2, blocks, ups = rpn(sd, "neck.", x1, return_all=True, **{k: v for k, v in nk.items() if k not in ("type", "logger")})
    pos = polar_pos_encoding(vg, hd.get("out_size_factor", 4)) if hd["type"] == "CenterHeadSinglePos" else None
    preds = center_head_single(sd, "bbox_head.", x2, hd["common_heads"], pos_encoding=pos)
    if return_stages:
        return preds, dict(features=feats, unq=unq, inv=inv, canvas=x1, blocks=blocks, ups=ups, x2=x2, pos=pos)
    return preds


# ======================================================================================
# T1  optimizer step of the training loop
#     OneCycle / annealing_cos            det3d/solver/learning_schedules_fastai.py:52-95
#     OptimWrapper.step (decoupled wd)    det3d/solver/fastai_optim.py:155-171
#     Adam(betas=(mom, 0.99))             det3d/torchie/apis/train.py:198-215 (torch.optim.Adam)
#     clip_grad_norm_(35, 2)              det3d/torchie/trainer/hooks/optimizer.py:10-13
# ======================================================================================
def one_cycle(step: int, total_step: int, lr_max: float, moms, div_factor: float, pct_start: float):
    """-> (lr, mom) the scheduler sets before optimizer step ``step`` (0-based)."""
    a1 = int(total_step * pct_start)
    low = lr_max / div_factor

    def cos(start, end, pct):
        return end + (start - end) / 2 * (np.cos(np.pi * pct) + 1)

    if step >= a1:  # the last phase whose start has been reached wins
        pct = (step - a1) / (total_step - a1)
        return cos(lr_max, low / 1e4, pct), cos(moms[1], moms[0], pct)
    pct = step / a1
    return cos(low, lr_max, pct), cos(moms[0], moms[1], pct)


def grad_clip_coef(total_norm: float, max_norm: float) -> float:
    """torch.nn.utils.clip_grad_norm_: grads *= min(1, max_norm / (total_norm + 1e-6))"""
    return min(1.0, max_norm / (total_norm + 1e-6))


def adam_decoupled_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, t: int, lr: float, beta1: float, beta2=0.99, eps=1e-8,
                        wd=0.01) -> None:
    """in place, fp32: p *= 1 - wd*lr (OptimWrapper.step), then torch.optim.Adam's single-tensor update
    with weight_decay 0; ``t`` is the 1-based step count of this parameter."""
    p.mul_(1 - wd * lr)
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** t
    bc2 = 1 - beta2 ** t
    denom = (v.sqrt() / (bc2 ** 0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))


# ======================================================================================
# H3  E2ESWVoteHead (geometry-aware head)   det3d/models/bbox_heads/e2e_swv_head.py:22-201
#     SwinTransformer / BasicLayer / SwinTransformerBlock / WindowAttention / PatchEmbed
#                                           det3d/models/bbox_heads/swin_utils/sw2votev4_util.py:42-419
# PARITY PARTLY PINNED: the head as a whole cannot be constructed or run in the reference (SURVEY F3:
# unregistered, typos such as `kernal_size`, `.contiuous()`, `torch.maixmum`, undefined names,
# layers never appended), but these parts of sw2votev4_util.py DO execute and are pinned by
# tests/golden/swv_fragments.npz (generated from the reference by make_golden.py::gen_swv_fragments,
# checked by tests/test_oracle_swv_fragments.py and, for the HIP path, tests/test_hip_swv.py):
#   PINNED to reference outputs
#     window_partition / window_reverse  :28-39    -> _window_partition / _window_reverse
#     MLP.forward                        :19-25    -> swv_mlp
#     PatchEmbed.forward (1 x 1 + LN)    :405-419  -> swv_patch_embed
#     SwinTransformerBlock.forward       :125-188  -> swv_swin_block: norm1, zero padding to window multiples (padded tokens
#                                                     are KEYS), cyclic shift, partition, reverse, shift back, crop, residual,
#                                                     norm2 + MLP + residual -- run in the reference around a stand-in
#                                                     attention (masked uniform average = the real attention at q = k = 0,
#                                                     v = x, proj = I, vote / position MLPs zero)
#   REPAIRS (the build's reading; not executable in the reference, HIP-vs-oracle only)
#     WindowAttention.__init__ / forward :42-103   -> swv_window_attention (cosine attention / clamp(tau), rpe MLP, vote embedding)
#     BasicLayer.forward's shift mask    :262-276  -> _swin_shift_mask (the reference fills a BOOL image and subtracts bool tensors)
#     SwinTransformer wiring             :331-353  -> e2e_swv_head (one BasicLayer + norm0), E2ESWVoteHead.__init__ / forward
#                                                     (e2e_swv_head.py:22-201: head branches, offset grid)
# The repaired reading of the intended computation:
#   * key names follow the config file (`kernel_size`, `sl_depth`, `weight_dict`);
#   * SwinTransformer = PatchEmbed(1x1 conv + LayerNorm) + ONE BasicLayer(depth 2, shift 0 / 3)
#     + LayerNorm `norm0` (sw2votev4_util.py:331-353 builds the layer but never appends it);
#   * WindowAttention: `x = (attn @ v).transpose(1, 2).reshape(B_, N, C)` (B is undefined at :98);
#   * cls_head = 2 x (Conv3x3 + BN + ReLU) + Conv3x3 -> classes (e2e_swv_head.py:76-86 rebuilds the
#     Sequential inside the loop with mismatching channel counts);
#   * offset_grid: x, y = grid_size[:2] // out_size_factor element-wise (:176 divides a list).
# ======================================================================================
def swv_offset_grid(grid_size, out_size_factor, min_volume_space, max_volume_space) -> Tensor:
    """(1,2,Y,X) Cartesian cell-centre coordinates of the polar BEV map (e2e_swv_head.py:175-192):
    x = range axis, y = azimuth axis; cart = (r cos a, r sin a)."""
    x, y = int(grid_size[0]) // out_size_factor, int(grid_size[1]) // out_size_factor
    xmin, ymin = float(min_volume_space[0]), float(min_volume_space[1])
    xmax, ymax = float(max_volume_space[0]), float(max_volume_space[1])
    xoff, yoff = (xmax - xmin) / x, (ymax - ymin) / y
    yv, xv = torch.meshgrid(torch.arange(y), torch.arange(x), indexing="ij")
    yv = (yv.float() + 0.5) * yoff + ymin
    xv = (xv.float() + 0.5) * xoff + xmin
    return torch.stack([xv * torch.cos(yv), xv * torch.sin(yv)], 0)[None]


def _swin_shift_mask(Hp: int, Wp: int, ws: int, shift: int) -> Tensor:
    """(nW, ws*ws, ws*ws) additive mask of BasicLayer.forward (sw2votev4_util.py:259-276)"""
    img = torch.zeros((1, Hp, Wp, 1))
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, h, w, :] = cnt
            cnt += 1
    mw = _window_partition(img, ws).view(-1, ws * ws)
    am = mw.unsqueeze(1) - mw.unsqueeze(2)
    return am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0)


def _window_partition(x: Tensor, ws: int) -> Tensor:
    B, H, W, C = x.shape
    x = x.view(B, H // ws, ws, W // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)


def _window_reverse(win: Tensor, ws: int, H: int, W: int) -> Tensor:
    B = int(win.shape[0] / (H * W / ws / ws))
    x = win.view(B, H // ws, W // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def swv_mlp(sd: SD, p: str, x: Tensor) -> Tensor:
    """MLP.forward (sw2votev4_util.py:19-25), dropout off; pinned by swv_fragments.npz"""
    return F.linear(F.gelu(F.linear(x, sd[p + "fc1.weight"], sd[p + "fc1.bias"])), sd[p + "fc2.weight"], sd[p + "fc2.bias"])


def swv_patch_embed(sd: SD, p: str, x: Tensor) -> Tensor:
    """PatchEmbed.forward with patch_size 1 and LayerNorm (sw2votev4_util.py:405-419): (B, Cin, H, W) -> tokens (B, H*W, C);
    pinned by swv_fragments.npz"""
    t = F.conv2d(x, sd[p + "proj.weight"], sd[p + "proj.bias"]).flatten(2).transpose(1, 2)
    return F.layer_norm(t, (t.shape[-1],), sd[p + "norm.weight"], sd[p + "norm.bias"])


def swv_window_attention(sd: SD, p: str, x: Tensor, mask, pos: Tensor, vote: Tensor, heads: int) -> Tensor:
    """WindowAttention.forward (sw2votev4_util.py:65-103): cosine attention / clamp(tau), relative position
    bias MLP on pairwise Cartesian offsets, vote embedding added to q, k and v.
    x (B_,N,C); pos (B_,N,2); vote (B_,N,3)."""
    B_, N, C = x.shape
    d = C // heads
    ve = F.conv1d(F.relu(F.conv1d(vote.permute(0, 2, 1).contiguous(), sd[p + "vote_mlp.0.weight"], sd[p + "vote_mlp.0.bias"])),
                  sd[p + "vote_mlp.2.weight"], sd[p + "vote_mlp.2.bias"])           # (B_, C, N)
    ve = ve.reshape(B_, heads, d, N).permute(0, 1, 3, 2)
    qkv = F.linear(x, sd[p + "qkv.weight"], sd.get(p + "qkv.bias")).reshape(B_, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] + ve, qkv[1] + ve, qkv[2] + ve
    nq, nk = q.norm(dim=-1, keepdim=True), k.norm(dim=-1, keepdim=True)
    attn = torch.einsum("bhnd,bhmd->bhnm", q, k) / torch.maximum(nq * nk.transpose(-2, -1), torch.tensor(1e-6))
    attn = attn / sd[p + "tau"].clamp(min=0.01)
    pe = pos.permute(0, 2, 1).contiguous()
    rel = pe[:, :, :, None] - pe[:, :, None, :]                                        # (B_, 2, N, N)
    rpe = F.conv2d(F.relu(F.conv2d(rel, sd[p + "rpe.0.weight"], sd[p + "rpe.0.bias"])), sd[p + "rpe.2.weight"], sd[p + "rpe.2.bias"])
    attn = attn + rpe
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.view(B_ // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    attn = attn.softmax(dim=-1)
    out = (attn @ v).transpose(1, 2).reshape(B_, N, C)
    return F.linear(out, sd[p + "proj.weight"], sd[p + "proj.bias"])


def swv_swin_block(sd: SD, p: str, x: Tensor, H: int, W: int, pos: Tensor, vote: Tensor, ws: int, shift: int, heads: int) -> Tensor:
    """SwinTransformerBlock.forward (sw2votev4_util.py:127-188); x (B, H*W, C), pos (B,H*W,2), vote (B,H*W,3)"""
    B, L, C = x.shape
    shortcut = x
    y = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"]).view(B, H, W, C)
    pr, pb = (ws - W % ws) % ws, (ws - H % ws) % ws
    y = F.pad(y, [0, 0, 0, pr, 0, pb])
    pe = F.pad(pos.view(B, H, W, 2), [0, 0, 0, pr, 0, pb])
    vo = F.pad(vote.view(B, H, W, 3), [0, 0, 0, pr, 0, pb])
    Hp, Wp = y.shape[1], y.shape[2]
    mask = None
    if shift > 0:
        y, pe, vo = (torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) for t in (y, pe, vo))
        mask = _swin_shift_mask(Hp, Wp, ws, shift)
    yw = _window_partition(y, ws).view(-1, ws * ws, C)
    pw = _window_partition(pe, ws).view(-1, ws * ws, 2)
    vw = _window_partition(vo, ws).view(-1, ws * ws, 3)
    aw = swv_window_attention(sd, p + "attn.", yw, mask, pw, vw, heads)
    y = _window_reverse(aw.view(-1, ws, ws, C), ws, Hp, Wp)
    if shift > 0:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    y = y[:, :H, :W, :].contiguous().view(B, H * W, C)
    x = shortcut + y
    z = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    return x + swv_mlp(sd, p + "mlp.", z)


def e2e_swv_head(sd: SD, prefix: str, x: Tensor, offset_grid: Tensor, window=7, depth=2, heads=4, iou=True,
                 return_feat=False, train=False) -> Dict[str, Tensor]:
    """E2ESWVoteHead.forward (e2e_swv_head.py:150-173); BatchNorm2d with the running statistics, or (train) the batch statistics"""
    p = prefix

    def conv(name, t, pad=1):
        return F.conv2d(t, sd[p + name + ".weight"], sd.get(p + name + ".bias"), padding=pad)

    def bn(name, t):
        return _bn(sd, p + name + ".", t, train, eps=1e-5, momentum=0.1)

    centers = conv("vote_head.2", F.relu(conv("vote_head.0", x)))
    vote_cls = conv("vote_cls_head.3", F.relu(bn("vote_cls_head.1", conv("vote_cls_head.0", x))))
    B, _, H, W = x.shape
    pos = offset_grid.expand(B, -1, -1, -1).flatten(2).transpose(1, 2)                  # (B, HW, 2)
    vote = torch.cat([centers, vote_cls], 1).flatten(2).transpose(1, 2)                 # (B, HW, 3)
    lp = p + "layer."
    t = swv_patch_embed(sd, lp + "patch_embed.", x)
    C = t.shape[-1]
    for i in range(depth):
        t = swv_swin_block(sd, f"{lp}layers.0.blocks.{i}.", t, H, W, pos, vote, window, 0 if i % 2 == 0 else window // 2, heads)
    t = F.layer_norm(t, (C,), sd[lp + "norm0.weight"], sd[lp + "norm0.bias"])
    feat = t.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    h = feat
    for i in range(2):
        h = F.relu(bn(f"cls_head.{i}.1", conv(f"cls_head.{i}.0", h)))
    hm = conv("cls_head.2", h)
    boxes = conv("bbox_head.2", F.relu(conv("bbox_head.0", feat)))
    ret = dict(pred_centers=centers, pred_vote_cls=vote_cls, hm=hm, reg=boxes[:, :2], height=boxes[:, 2:3], dim=boxes[:, 3:6], rot=boxes[:, 6:8])
    if iou:
        ret["iou"] = conv("iou_head.2", F.relu(conv("iou_head.0", feat)))
    if return_feat:
        ret["feat"] = feat
    return ret


# ======================================================================================
# next-2  decode + rotated NMS            det3d/models/bbox_heads/center_head.py:350-402 (decode),
#                                         :462-577 (post_processing), :404-460 (predict)
#         rotate_nms_pcdet                det3d/core/bbox/box_torch_ops.py:248-277
#         BEV rotated IoU / greedy NMS    det3d/ops/iou3d_nms/src/iou3d_nms_kernel.cu:104-311, iou3d_nms.cpp:90-136
# The IoU / NMS arithmetic is restated in oracle/box_nms.c (the reference's is CUDA only: PARITY UNPINNED,
# see that file's header); this part is the numpy restatement of the decode and of the selection logic
# for the plain path (no double flip, no stateful / per-class NMS, no panoptic, sector 0).
# ======================================================================================
def double_flip_merge(preds: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """CenterHead.double_flip_decode (center_head.py:289-346): NHWC arrays (4B, H, W, c) in groups [original, y -> -y, x -> -x, both]
    -> merged (B, H, W, c); 'hm' comes out as averaged probabilities, 'dim' as averaged sizes.  Pinned by tests/golden/double_flip.npz."""
    out = {}
    g = {}
    for k, v in preds.items():
        n, H, W, C = v.shape
        t = torch.from_numpy(np.ascontiguousarray(v)).float().reshape(n // 4, 4, H, W, C).clone()
        t[:, 1] = torch.flip(t[:, 1], dims=[1])
        t[:, 2] = torch.flip(t[:, 2], dims=[2])
        t[:, 3] = torch.flip(t[:, 3], dims=[1, 2])
        g[k] = t
    out["hm"] = torch.sigmoid(g["hm"]).mean(dim=1)
    out["dim"] = torch.exp(g["dim"]).mean(dim=1)
    out["height"] = g["height"].mean(dim=1)
    reg = g["reg"]
    reg[:, 1, ..., 1] = 1 - reg[:, 1, ..., 1]
    reg[:, 2, ..., 0] = 1 - reg[:, 2, ..., 0]
    reg[:, 3, ..., 0] = 1 - reg[:, 3, ..., 0]
    reg[:, 3, ..., 1] = 1 - reg[:, 3, ..., 1]
    out["reg"] = reg.mean(dim=1)
    rots, rotc = g["rot"][..., 0:1], g["rot"][..., 1:2]
    rotc[:, 1] *= -1
    rots[:, 2] *= -1
    rots[:, 3] *= -1
    rotc[:, 3] *= -1
    out["rot"] = torch.cat([rots.mean(dim=1), rotc.mean(dim=1)], -1)
    if "vel" in g:
        vel = g["vel"]
        vel[:, 1, ..., 1] *= -1
        vel[:, 2, ..., 0] *= -1
        vel[:, 3] *= -1
        out["vel"] = vel.mean(dim=1)
    return {k: v.numpy() for k, v in out.items()}


def center_decode(preds: Dict[str, np.ndarray], voxel_shape: str, out_size_factor, voxel_size, pc_range, rectify=False, activated=False):
    """preds: NHWC numpy arrays (B,H,W,c) 'hm','reg','height','dim','rot'[,'vel'] (raw head outputs; activated: the merged maps of
    double_flip_merge, whose hm / dim are probabilities / sizes already, center_head.py:350-353).
    -> boxes (B, H*W, 9 or 7) [x, y, z, dims(3), (vel 2), rot], scores (B, H*W, ncls) (center_head.py:350-402)"""
    hm = preds["hm"].astype(np.float32) if activated else 1.0 / (1.0 + np.exp(-preds["hm"].astype(np.float32)))
    dim = preds["dim"].astype(np.float32) if activated else np.exp(preds["dim"].astype(np.float32))
    rot = np.arctan2(preds["rot"][..., 0:1], preds["rot"][..., 1:2]).astype(np.float32)
    B, H, W, ncls = hm.shape
    reg = preds["reg"].reshape(B, H * W, 2).astype(np.float32)
    hei = preds["height"].reshape(B, H * W, 1).astype(np.float32)
    rot = rot.reshape(B, H * W, 1)
    dim = dim.reshape(B, H * W, 3)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    xs, ys = xs.reshape(1, -1, 1), ys.reshape(1, -1, 1)
    if voxel_shape == "cylinder":
        rho = xs * np.float32(out_size_factor) * np.float32(voxel_size[0]) + np.float32(pc_range[0])
        az = ys * np.float32(out_size_factor) * np.float32(voxel_size[1]) + np.float32(pc_range[1])
        cx, cy = rho * np.cos(az), rho * np.sin(az)
        x, y = cx + reg[:, :, 0:1], cy + reg[:, :, 1:2]
        azs = None
        if rectify:
            azs = np.arctan2(y, x)
            rot = rot + azs
    else:
        x = (xs + reg[:, :, 0:1]) * np.float32(out_size_factor) * np.float32(voxel_size[0]) + np.float32(pc_range[0])
        y = (ys + reg[:, :, 1:2]) * np.float32(out_size_factor) * np.float32(voxel_size[1]) + np.float32(pc_range[1])
    parts = [x, y, hei, dim]
    if "vel" in preds:
        vel = preds["vel"].reshape(B, H * W, 2).astype(np.float32).copy()
        if voxel_shape == "cylinder" and rectify:
            vr = np.linalg.norm(vel, axis=-1)
            va = np.arctan2(vel[:, :, 1], vel[:, :, 0]) + azs[..., 0]
            vel = np.stack([vr * np.cos(va), vr * np.sin(va)], -1)
        parts.append(vel)
    parts.append(rot)
    return np.concatenate([p.astype(np.float32) for p in parts], 2), hm.reshape(B, H * W, ncls)


def swv_decode(preds: Dict[str, np.ndarray], offset_grid: np.ndarray, iou_factor: int = 1, rectify: bool = False):
    """E2ESWVoteHead.decode (e2e_swv_head.py:313-366; the reference's code does not run -- restated from its text, PARITY UNPINNED).
    preds: NHWC numpy (B,H,W,c) 'hm','reg','height','dim','rot'[,'iou']; offset_grid (2,H,W) Cartesian cell centres.
    -> boxes (B, H*W, 7) [x, y, z, dims(3), rot], scores (B, H*W, ncls)"""
    f = np.float32
    hm = (1.0 / (1.0 + np.exp(-preds["hm"].astype(f)))).astype(f)
    B, H, W, ncls = hm.shape
    if "iou" in preds:
        u = np.clip((preds["iou"].astype(f) + f(1.0)) * f(0.5), f(0.0), f(1.0))
        hm = hm * (u if iou_factor == 1 else np.power(u, f(iou_factor))).astype(f)
    dim = np.exp(preds["dim"].astype(f)).reshape(B, H * W, 3)
    rot = np.arctan2(preds["rot"][..., 1:2], preds["rot"][..., 0:1]).astype(f).reshape(B, H * W, 1)
    g = np.asarray(offset_grid, f).reshape(2, H * W)
    reg = preds["reg"].reshape(B, H * W, 2).astype(f)
    x, y = reg[:, :, 0:1] + g[0][None, :, None], reg[:, :, 1:2] + g[1][None, :, None]
    if rectify:
        rot = rot + np.arctan2(y, x).astype(f)
        rot = rot + np.where(rot > f(np.pi), f(-2 * np.pi), np.where(rot < f(-np.pi), f(2 * np.pi), f(0.0))).astype(f)
    hei = preds["height"].reshape(B, H * W, 1).astype(f)
    return np.concatenate([x, y, hei, dim, rot], 2).astype(f), hm.reshape(B, H * W, ncls)


def nms_boxes_pcdet(boxes: np.ndarray) -> np.ndarray:
    """(n, >=7) [x,y,z,l,w,h,...,rot] -> (n,7) in the NMS kernel's convention (box_torch_ops.py:255-257)"""
    b = boxes[:, [0, 1, 2, 4, 3, 5, -1]].astype(np.float32).copy()
    b[:, -1] = -b[:, -1] - np.float32(np.pi / 2)
    return b


def center_post_process(boxes: np.ndarray, hm: np.ndarray, score_threshold: float, post_center_range, nms_iou_threshold: float,
                        nms_pre_max_size: int, nms_post_max_size: int, nms_fn, per_class: bool = False):
    """one sample of post_processing (center_head.py:470-520, plain path).  nms_fn(sorted boxes (n,7), thresh) -> kept
    indices (the C oracle's ov_nms_sorted).  Ties in the score sort are broken by cell index (torch.sort leaves them
    unspecified).  -> dict(box3d_lidar, scores, label_preds, cells)

    per_class (test_cfg.per_class_nms, center_head.py:514-518): detectron2's layers.batched_nms_rotated -- THIRD PARTY, absent
    here, parity unpinned.  Its published semantics: every class is moved to its own region of the plane, one greedy rotated
    NMS in score order runs over all boxes, the kept indices come back in score order; i.e. a greedy NMS in which only boxes
    of the same class suppress each other.  The BEV rectangle it is given, (x, y, dims[0], dims[1], rot in degrees) in
    detectron2's convention, is the rectangle of nms_boxes_pcdet (dims[0] along the direction -rot).  Restated with the same
    IoU routine as the multi-class path; nms_pre_max_size bounds the candidates (the reference passes all of them)."""
    scores, labels = hm.max(-1), hm.argmax(-1)
    pr = np.asarray(post_center_range, np.float32)
    mask = (scores > np.float32(score_threshold)) & (boxes[:, :3] >= pr[:3]).all(1) & (boxes[:, :3] <= pr[3:]).all(1)
    cells = np.nonzero(mask)[0]
    b, s, l = boxes[cells], scores[cells], labels[cells]
    order = np.lexsort((cells, -s))[:nms_pre_max_size]
    if per_class:
        lab, kept = l[order], []
        for c in np.unique(lab):
            idx = np.nonzero(lab == c)[0]                       # positions in the score order
            kept.append(idx[np.asarray(nms_fn(nms_boxes_pcdet(b[order[idx]]), nms_iou_threshold), np.int64)])
        keep = np.sort(np.concatenate(kept)) if kept else np.zeros(0, np.int64)
    else:
        keep = np.asarray(nms_fn(nms_boxes_pcdet(b[order]), nms_iou_threshold), np.int64)
    sel = order[keep][:nms_post_max_size]
    return dict(box3d_lidar=b[sel], scores=s[sel], label_preds=l[sel], cells=cells[sel])


def center_post_process_stateful(boxes: np.ndarray, hm: np.ndarray, score_threshold: float, post_center_range, nms_iou_threshold: float,
                                 nms_pre_max_size: int, nms_post_max_size: int, nms_fn, prev, sector_angle: float, sec_id: int):
    """one sample of post_processing with test_cfg.stateful_nms (center_head.py:470-531): threshold / range mask, the sector's candidates
    rotated into the sweep's frame, the previous sectors' detections (prev: dict(box3d_lidar, scores, label_preds) or None) put in front,
    ONE rotated NMS over the union, at most nms_post_max_size * (sec_id + 1) boxes.  Ties in the score sort: the sector's own cells
    first (by cell index), carried-over detections after (index H*W + k) -- torch leaves them unspecified.
    -> dict(box3d_lidar, scores, label_preds, cells)"""
    scores, labels = hm.max(-1), hm.argmax(-1)
    pr = np.asarray(post_center_range, np.float32)
    mask = (scores > np.float32(score_threshold)) & (boxes[:, :3] >= pr[:3]).all(1) & (boxes[:, :3] <= pr[3:]).all(1)
    cells = np.nonzero(mask)[0]
    b, s, l = boxes[cells].copy(), scores[cells], labels[cells]
    if prev is not None:
        c, sn = np.float32(np.cos(sector_angle)), np.float32(np.sin(-sector_angle))
        m = np.array([[c, -sn], [sn, c]], np.float32)           # rot_mat_T of the reference: [[cos, -sin(-a)], [sin(-a), cos]]
        xy = b[:, :2].copy()
        b[:, 0] = xy[:, 0] * m[0, 0] + xy[:, 1] * m[1, 0]
        b[:, 1] = xy[:, 0] * m[0, 1] + xy[:, 1] * m[1, 1]
        b[:, -1] -= np.float32(sector_angle)
        if b.shape[1] > 7:
            v = b[:, 6:8].copy()
            b[:, 6] = v[:, 0] * m[0, 0] + v[:, 1] * m[1, 0]
            b[:, 7] = v[:, 0] * m[0, 1] + v[:, 1] * m[1, 1]
        npv = len(prev["scores"])
        idx = np.concatenate([cells, len(scores) + np.arange(npv)])
        b = np.concatenate([b, np.asarray(prev["box3d_lidar"], np.float32)], 0)
        s = np.concatenate([s, np.asarray(prev["scores"], np.float32)])
        l = np.concatenate([l, np.asarray(prev["label_preds"], np.int64)])
    else:
        idx = cells
    order = np.lexsort((idx, -s))[:nms_pre_max_size]
    keep = np.asarray(nms_fn(nms_boxes_pcdet(b[order]), nms_iou_threshold), np.int64)
    sel = order[keep][:nms_post_max_size * (sec_id + 1)]
    return dict(box3d_lidar=b[sel], scores=s[sel], label_preds=l[sel], cells=idx[sel])


# ======================================================================================
# next-1  SpMiddleResNetFHD (sparse 3-D middle encoder)   det3d/models/backbones/scn.py:17-192
# PARITY UNPINNED: the arithmetic of SubMConv3d / SparseConv3d / SparseConvTensor.dense is the third-party spconv
# package (README.md:45 `spconv-cu114`, unpinned), which is not installed here and has no CPU path in the reference.
# Restated from spconv's published semantics on DENSE tensors with an explicit activity mask:
#   SubMConv3d      y = conv3d(x, W, b, padding=k//2) at the ACTIVE INPUT sites only (the active set is unchanged)
#   SparseConv3d    y = conv3d(x, W, None, stride, padding); active outputs = sites whose receptive field holds an
#                   active input (max-pool of the mask)
#   BatchNorm1d / ReLU act on active features only; inactive sites stay exactly zero in .dense()
# Weight layout of spconv 2.x: (Cout, kD, kH, kW, Cin).
# ======================================================================================
def _sp_w(w: Tensor) -> Tensor:
    return w.permute(0, 4, 1, 2, 3).contiguous()


def _sp_bn(sd: SD, p: str, x: Tensor, mask: Tensor, eps=1e-3, train=False) -> Tensor:
    """BatchNorm1d over the ACTIVE sites' feature rows; train: batch statistics (biased variance) of those rows, running buffers
    untouched"""
    if train:
        n = mask.sum()
        mean = (x * mask).sum(dim=(0, 2, 3, 4)) / n
        var = (((x - mean[None, :, None, None, None]) ** 2) * mask).sum(dim=(0, 2, 3, 4)) / n
        y = (x - mean[None, :, None, None, None]) / torch.sqrt(var[None, :, None, None, None] + eps)
        return (y * sd[p + "weight"][None, :, None, None, None] + sd[p + "bias"][None, :, None, None, None]) * mask
    y = (x - sd[p + "running_mean"][None, :, None, None, None]) / torch.sqrt(sd[p + "running_var"][None, :, None, None, None] + eps)
    return (y * sd[p + "weight"][None, :, None, None, None] + sd[p + "bias"][None, :, None, None, None]) * mask


def _sp_subm(sd: SD, p: str, x: Tensor, mask: Tensor) -> Tensor:
    w = _sp_w(sd[p + "weight"])
    return F.conv3d(x, w, sd.get(p + "bias"), padding=[k // 2 for k in w.shape[2:]]) * mask


def _sp_down(sd: SD, p: str, x: Tensor, mask: Tensor, stride, padding):
    w = _sp_w(sd[p + "weight"])
    k = list(w.shape[2:])
    m = (F.max_pool3d(mask, k, stride, padding) > 0).to(x.dtype)
    return F.conv3d(x, w, None, stride, padding) * m, m


def _sp_block(sd: SD, p: str, x: Tensor, mask: Tensor, train=False) -> Tensor:
    out = F.relu(_sp_bn(sd, p + "bn1.", _sp_subm(sd, p + "conv1.", x, mask), mask, train=train))
    out = _sp_bn(sd, p + "bn2.", _sp_subm(sd, p + "conv2.", out, mask), mask, train=train)
    return F.relu(out + x)


def sp_middle_resnet_fhd(sd: SD, prefix: str, voxel_features: Tensor, coors: np.ndarray, batch_size: int, input_shape,
                         extra_sp_shape=(1, 0, 0), return_stages=False, train=False):
    """voxel_features (V,C); coors (V,4) int [b,z,y,x]; input_shape [x,y,z] -> (B, C*D, H, W) dense BEV map (scn.py:157-192);
    train: every BatchNorm1d uses the batch statistics of the active rows (module.train())"""
    D, H, W = (int(v) + e for v, e in zip(list(input_shape)[::-1], extra_sp_shape))
    C = voxel_features.shape[1]
    x = torch.zeros((batch_size, C, D, H, W), dtype=voxel_features.dtype)
    mask = torch.zeros((batch_size, 1, D, H, W), dtype=voxel_features.dtype)
    c = torch.from_numpy(np.asarray(coors)).long()
    x[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = voxel_features
    mask[c[:, 0], 0, c[:, 1], c[:, 2], c[:, 3]] = 1.0
    p = prefix
    x = F.relu(_sp_bn(sd, p + "conv_input.1.", _sp_subm(sd, p + "conv_input.0.", x, mask), mask, train=train))
    for i in range(2):
        x = _sp_block(sd, f"{p}conv1.{i}.", x, mask, train)
    stages = [x]
    pad4 = 0 if extra_sp_shape[0] != 0 else 1
    for name, pad in (("conv2", [1, 1, 1]), ("conv3", [1, 1, 1]), ("conv4", [pad4, 1, 1])):
        x, mask = _sp_down(sd, f"{p}{name}.0.", x, mask, [2, 2, 2], pad)
        x = F.relu(_sp_bn(sd, f"{p}{name}.1.", x, mask, train=train))
        for i in (3, 4):
            x = _sp_block(sd, f"{p}{name}.{i}.", x, mask, train)
        stages.append(x)
    x, mask = _sp_down(sd, p + "extra_conv.0.", x, mask, [2, 1, 1], [0, 0, 0])
    x = F.relu(_sp_bn(sd, p + "extra_conv.1.", x, mask, train=train))
    N, Cc, Dd, Hh, Ww = x.shape
    ret = x.reshape(N, Cc * Dd, Hh, Ww)
    return (ret, stages) if return_stages else ret


# ======================================================================================
# next-3  CenterPoint target assignment on the polar grid
#         AssignLabel.assign_heatmap_polar   det3d/datasets/pipelines/preprocess.py:253-342
#         gaussian_radius / gaussian2D / draw_umich_gaussian   det3d/core/utils/center_utils.py:18-64
#         center_to_corner_box2d             det3d/core/bbox/box_np_ops.py:265-285 (corners_nd :55-85, rotation_2d :207-220)
# Pinned by tests/golden/assign.npz (captured from the reference).  dtypes as the pipeline delivers them: float32 boxes,
# float32 voxel_size / pc_range (VoxelGenerator), so the cell arithmetic is float32 and only the real-world cell centre
# (int32 * float32 under NumPy's promotion rules) is float64.
# ======================================================================================
def gaussian_radius_f32(h: np.float32, w: np.float32, min_overlap: float) -> np.float32:
    f = np.float32
    b1 = h + w
    c1 = w * h * f(1 - min_overlap) / f(1 + min_overlap)
    r1 = (b1 + np.sqrt(b1 * b1 - f(4) * c1)) / f(2)
    b2 = f(2) * (h + w)
    c2 = f(1 - min_overlap) * w * h
    r2 = (b2 + np.sqrt(b2 * b2 - f(16) * c2)) / f(2)
    a3 = f(4 * min_overlap)
    b3 = f(-2 * min_overlap) * (h + w)
    c3 = f(min_overlap - 1) * w * h
    r3 = (b3 + np.sqrt(b3 * b3 - f(4) * a3 * c3)) / f(2)
    return min(r1, r2, r3)


def assign_heatmap_polar(gt_boxes: np.ndarray, gt_classes: np.ndarray, ncls: int, max_objs: int, out_size_factor: int,
                         gaussian_overlap: float, min_radius: int, rectify: bool, voxel_size, pc_range, feature_map_size):
    """gt_boxes (n, 9) f32 [x,y,z,l,w,h,vx,vy,rot]; gt_classes (n,) 1-based.  -> hm (ncls, A, R) f32, ind / mask / cat (max_objs,),
    anno_box (max_objs, 10) f32 [dx, dy, z, log l, log w, log h, vx, vy, sin, cos]."""
    f = np.float32
    vs, pr = np.asarray(voxel_size, f), np.asarray(pc_range, f)
    R, A = int(feature_map_size[0]), int(feature_map_size[1])
    hm = np.zeros((ncls, A, R), f)
    ind, mask, cat = np.zeros(max_objs, np.int64), np.zeros(max_objs, np.uint8), np.zeros(max_objs, np.int64)
    anno = np.zeros((max_objs, 10), f)
    n = min(len(gt_boxes), max_objs)
    unit = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]], f)     # clockwise from the minimum corner
    for k in range(n):
        b = gt_boxes[k].astype(f)
        # NB the reference rotates the footprint by COLUMN 6 of the box (preprocess.py:266): the heading for 7-column Waymo
        # boxes, but vx for the 9-column nuScenes boxes [x,y,z,l,w,h,vx,vy,rot] -- reproduced as is
        s, c = np.sin(b[6]), np.cos(b[6])
        loc = b[3:5][None, :] * unit                                               # (4, 2) f32
        cx = loc[:, 0] * c + loc[:, 1] * s + b[0]                                  # rotation_2d: [x, y] @ [[c, -s], [s, c]]
        cy = loc[:, 0] * (-s) + loc[:, 1] * c + b[1]
        rho, az = np.sqrt(cx * cx + cy * cy), np.arctan2(cy, cx)
        dr = (rho.max() - rho.min()) / vs[0] / f(out_size_factor)
        da = (az.max() - az.min()) / vs[1] / f(out_size_factor)
        if not (dr > 0 and da > 0):
            continue
        r, a = np.sqrt(b[0] * b[0] + b[1] * b[1]), np.arctan2(b[1], b[0])
        radius = max(int(min_radius), int(gaussian_radius_f32(dr, da, gaussian_overlap)) - int(r > 30))
        ct = np.array([(r - pr[0]) / vs[0] / f(out_size_factor), (a - pr[1]) / vs[1] / f(out_size_factor)], f)
        ci = ct.astype(np.int32)
        ci[1] = np.clip(ci[1], 0, A - 1)
        if not (0 <= ci[0] < R):
            continue
        # draw_umich_gaussian(hm[cls], ct, radius): centre from the UNCLIPPED ct, clipped window, element-wise maximum
        cls = int(gt_classes[k]) - 1
        x, y = int(ct[0]), int(ct[1])
        left, right = min(x, radius), min(R - x, radius + 1)
        top, bottom = min(y, radius), min(A - y, radius + 1)
        if right > -left and bottom > -top:
            sigma = (2 * radius + 1) / 6
            yy, xx = np.ogrid[-top:bottom, -left:right]
            g = np.exp(-(xx * xx + yy * yy) / (2 * sigma * sigma))
            win = hm[cls, y - top:y + bottom, x - left:x + right]
            if min(win.shape) > 0 and min(g.shape) > 0:
                np.maximum(win, g, out=win)
        r_real = np.float64(ci[0]) * out_size_factor * np.float64(vs[0]) + np.float64(pr[0])
        a_real = np.float64(ci[1]) * out_size_factor * np.float64(vs[1]) + np.float64(pr[1])
        xc, yc = r_real * np.cos(a_real), r_real * np.sin(a_real)
        vx, vy, rot = b[6], b[7], b[8]
        if rectify:
            rot = rot - a
            vr, va = np.sqrt(vx * vx + vy * vy), np.arctan2(vy, vx) - a
            vx, vy = vr * np.cos(va), vr * np.sin(va)
        cat[k], ind[k], mask[k] = cls, int(ci[1]) * R + int(ci[0]), 1
        anno[k] = np.array([np.float64(b[0]) - xc, np.float64(b[1]) - yc, b[2], np.log(b[3]), np.log(b[4]), np.log(b[5]), vx, vy,
                            np.sin(rot), np.cos(rot)], np.float64).astype(f)
    return hm, ind, mask, cat, anno


# ======================================================================================
# next-4 (device half)  multi-sweep accumulation
#         read_file / remove_close / read_sweep     det3d/datasets/pipelines/loading.py:42-84
#         LoadPointCloudFromFile.get_points          loading.py:216-250 (key frame first, then the sweeps; time lag column)
# Pinned by tests/golden/sweeps.npz (captured from the reference on temporary .bin files).
# ======================================================================================
def accumulate_sweeps(clouds: List[np.ndarray], transforms: np.ndarray, time_lags: np.ndarray, min_distance: float = 1.0) -> np.ndarray:
    """clouds[s]: (n_s, >=4) f32 raw points [x,y,z,intensity,...] of sweep s (s = 0 is the key frame); transforms (S,4,4) f64;
    -> (N', 5) f32 [x, y, z, intensity, time lag]"""
    out = [np.concatenate([clouds[0][:, :4].astype(np.float32), np.zeros((len(clouds[0]), 1), np.float32)], 1)]
    for s in range(1, len(clouds)):
        p = clouds[s][:, :4].astype(np.float32)
        keep = ~((np.abs(p[:, 0]) < min_distance) & (np.abs(p[:, 1]) < min_distance))   # in the sweep's own frame
        p = p[keep]
        hom = np.concatenate([p[:, :3].astype(np.float64), np.ones((len(p), 1))], 1)
        p[:, :3] = (hom @ np.asarray(transforms[s], np.float64).T)[:, :3].astype(np.float32)
        out.append(np.concatenate([p, np.full((len(p), 1), np.float32(time_lags[s]), np.float32)], 1))
    return np.concatenate(out, 0)


# ======================================================================================
# V4 static twin  PillarFeatureNet.forward / PFNLayer.forward_static   det3d/models/readers/pillar_encoder.py:131-169, 47-60
# Pinned by tests/golden/pillar_static.npz (captured from the reference).
# ======================================================================================
def pillar_feature_net_static(sd: SD, prefix: str, voxels: Tensor, num_points: Tensor, coors: Tensor, voxel_size, pc_range,
                              with_distance=False, eps=1e-3) -> Tensor:
    """voxels (V,P,F), num_points (V,), coors (V,4) [b,z,y,x] -> (V, C_last); eval-mode BatchNorm1d"""
    vx, vy = voxel_size[0], voxel_size[1]
    xo, yo = vx / 2 + pc_range[0], vy / 2 + pc_range[1]
    mean = voxels[:, :, :3].sum(dim=1, keepdim=True) / num_points.to(voxels.dtype).view(-1, 1, 1)
    parts = [voxels, voxels[:, :, :3] - mean,
             torch.stack([voxels[:, :, 0] - (coors[:, 3].to(voxels.dtype).unsqueeze(1) * vx + xo),
                          voxels[:, :, 1] - (coors[:, 2].to(voxels.dtype).unsqueeze(1) * vy + yo)], -1)]
    if with_distance:
        parts.append(voxels[:, :, :3].norm(dim=2, keepdim=True))
    x = torch.cat(parts, -1)
    x = x * (torch.arange(voxels.shape[1])[None, :] < num_points[:, None]).to(x.dtype).unsqueeze(-1)   # padded slots -> 0
    n_layers = len([k for k in sd if k.startswith(prefix + "pfn_layers.") and k.endswith("linear.weight")])
    for i in range(n_layers):
        p = f"{prefix}pfn_layers.{i}."
        y = x @ sd[p + "linear.weight"].t()
        y = (y - sd[p + "norm.running_mean"]) / torch.sqrt(sd[p + "norm.running_var"] + eps) * sd[p + "norm.weight"] + sd[p + "norm.bias"]
        y = F.relu(y)
        ymax = y.max(dim=1, keepdim=True)[0]          # padded slots take part (relu of the BatchNorm shift), as in the reference
        x = ymax if i == n_layers - 1 else torch.cat([y, ymax.expand(-1, y.shape[1], -1)], 2)
    return x.squeeze(1)
