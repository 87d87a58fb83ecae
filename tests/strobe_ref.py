"""Host restatement (numpy / torch on the CPU) of the three device pieces of Cartesian sector streaming, written from their description
in include/partner_hip.h, and the seeded inputs the STROBE goldens and tests share.  Used to cross-check shapes that are not in
tests/golden/strobe.npz; the golden itself comes from the reference's own code (tests/golden/make_golden_strobe.py).

  split_cart_sectors   the sectors of cuboid points [x, y, z, ..., rho, phi]: rows, shifted azimuth, x / y, [z, y, x] cells, row indices
  memory_build         the whole-frame memory of a level from its stacked sector maps
  memory_read          the memory resampled into every sector's frame
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

CART_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
CART_VOXEL = (1.6, 1.6, 8.0)          # full grid 64 x 64, the 4-sector grid 32 x 32
SPLIT_SEEDS, SPLIT_POINTS = (300, 301), (2500, 2600)
SWEEP_SEEDS, SWEEP_POINTS = ((310, 311), (320, 321), (330, 331)), (800, 900)
SWEEP_ANGLES = ((0.04, -0.06), (-0.03, 0.05), (0.0, 0.0))       # ego rotation of each sweep's two samples (the last sweep's is not read)
RPN_SAMPLES = (0, 5)                  # the stacked samples of sweep 1 whose warped maps are stored in full for the RPNUber test
MEMORY_CASES = {                      # tag: (nsectors, batch, h, w, c, ego angles or None for the identity, seed)
    "m2": (2, 2, 8, 16, 4, (0.07, -0.11), 41),
    "m1": (1, 2, 16, 16, 4, (0.05, -0.09), 42),
    "m4id": (4, 1, 16, 16, 4, None, 43),
}


def cuboid_sweep(n: int, seed: int, special: bool = False) -> np.ndarray:
    """(n, 7) float32 [x, y, z, i, t, rho, phi]: a synthetic sweep as transform_points(pc, 'cuboid') leaves it.  ``special``: no point
    with an azimuth in [0, pi / 2) (the third of four sectors stays empty) and three points exactly at phi = -pi"""
    r = np.random.default_rng(seed)
    rho, phi = r.uniform(1.0, 50.0, n), r.uniform(-np.pi, np.pi, n)
    if special:
        phi = np.where((phi >= 0) & (phi < np.pi / 2), phi - np.pi, phi)
    pc = np.stack([rho * np.cos(phi), rho * np.sin(phi), r.uniform(-3.0, 1.0, n), r.uniform(0.0, 1.0, n), np.zeros(n)], 1).astype(np.float32)
    if special:
        pc[:3, 0], pc[:3, 1] = [-7.5, -20.25, -44.0], -0.0
    rho32 = np.sqrt(pc[:, 0] ** 2 + pc[:, 1] ** 2)
    phi32 = np.arctan2(pc[:, 1], pc[:, 0])
    out = np.ascontiguousarray(np.hstack((pc, rho32[:, None], phi32[:, None])).astype(np.float32))
    if special:
        assert (out[:3, 6] == np.float32(-np.pi)).all() and not ((out[:, 6] >= 0) & (out[:, 6] < np.float32(np.pi / 2))).any()
    return out


def relu_maps(nsectors, batch, h, w, c, seed) -> torch.Tensor:
    """post-ReLU random maps (nsectors * batch, c, h, w): about half of the elements are exactly zero"""
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn((nsectors * batch, c, h, w), generator=g))


def rotations(angles, batch) -> torch.Tensor:
    if angles is None:
        return torch.eye(2).repeat(batch, 1, 1)
    return torch.tensor(np.stack([np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], np.float32) for a in angles]))


# ------------------------------------------------------------------------------------------------------------------------ split
def sector_grid(grid, nsectors):
    g = [int(v) for v in grid]
    return [g[0] // 2 if nsectors >= 4 else g[0], g[1] // 2 if nsectors >= 2 else g[1], g[2]]


def split_cart_sectors(points: np.ndarray, nsectors: int, pc_range=CART_RANGE, voxel_size=CART_VOXEL):
    """-> per sector (rows (k, f) float32, cells (k, 3) int64 [z, y, x], index (k,) int64 of the rows in ``points``).  The bounds and the shift
    are float64; the azimuth column is compared and shifted in float64 and rounded back to float32; cells in float32"""
    rg, vs = np.asarray(pc_range, np.float32), np.asarray(voxel_size, np.float32)
    grid = sector_grid(np.round((rg[3:] - rg[:3]) / vs).astype(np.int64), nsectors)
    phi64 = points[:, -1].astype(np.float64)
    interval = 2 * np.pi / nsectors
    out = []
    for i in range(nsectors):
        lo, hi = -np.pi + i * interval, -np.pi + (i + 1) * interval
        keep = np.ones(len(points), bool)
        if i > 0:
            keep &= phi64 >= lo
        if i < nsectors - 1:
            keep &= phi64 < hi
        idx = np.where(keep)[0]
        rows = points[idx].copy()
        rows[:, -1] = (phi64[idx] - (lo + np.pi)).astype(np.float32)
        rows[:, 0] = rows[:, -2] * np.cos(rows[:, -1])
        rows[:, 1] = rows[:, -2] * np.sin(rows[:, -1])
        q = (rows[:, :3] - rg[:3]) / vs
        cells = np.floor(np.clip(q, 0, np.asarray(grid, np.float32) - 1)).astype(np.int64)[:, ::-1]
        out.append((rows, np.ascontiguousarray(cells), idx))
    return out


def border_distance(rows: np.ndarray, pc_range=CART_RANGE, voxel_size=CART_VOXEL) -> np.ndarray:
    """per row the distance (metres) of x and y to the nearest cell border, the smaller of the two"""
    rg, vs = np.asarray(pc_range, np.float64), np.asarray(voxel_size, np.float64)
    q = (rows[:, :2].astype(np.float64) - rg[:2]) / vs[:2]
    return (np.abs(q - np.round(q)) * vs[:2]).min(1)


# ------------------------------------------------------------------------------------------------------------------------ memory
def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _region(nsectors, pc_range):
    x_lo, y_lo, x_hi, y_hi = pc_range[0], pc_range[1], pc_range[3], pc_range[4]
    return x_lo, y_lo, (0.0 if nsectors >= 4 else x_hi), (0.0 if nsectors >= 2 else y_hi)


def _corners(lo_x, lo_y, hi_x, hi_y, rows, cols):
    """(rows, cols, 2) float32 [x, y] of the cells' lower corners: pitch formed in float64, rounded once, times the float32 index"""
    gy, gx = torch.meshgrid(torch.arange(rows), torch.arange(cols), indexing="ij")
    x = _f32((hi_x - lo_x) / cols) * gx.float() + _f32(lo_x)
    y = _f32((hi_y - lo_y) / rows) * gy.float() + _f32(lo_y)
    return torch.stack([x, y], -1)


def _rot(j, nsectors):
    a = 2 * np.pi / nsectors * j
    return torch.tensor([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], dtype=torch.float32)


def _apply(mat, pts):
    """mat (.., 2, 2) on pts (.., 2): two rounded products and one rounded sum per coordinate, no fused multiply-add"""
    return torch.stack([mat[..., 0, 0] * pts[..., 0] + mat[..., 0, 1] * pts[..., 1], mat[..., 1, 0] * pts[..., 0] + mat[..., 1, 1] * pts[..., 1]], -1)


def memory_build(maps: torch.Tensor, rot: torch.Tensor, nsectors: int, pc_range=CART_RANGE) -> torch.Tensor:
    """maps (nsectors * B, C, h, w), rot (B, 2, 2) -> memory (B, C, H, W)"""
    n, c, h, w = maps.shape
    bs = n // nsectors
    H, W = h * (2 if nsectors >= 2 else 1), w * (2 if nsectors >= 4 else 1)
    x_lo, y_lo, mx, my = _region(nsectors, pc_range)
    p = _corners(pc_range[0], pc_range[1], pc_range[3], pc_range[4], H, W)
    q = _apply(rot.float()[:, None, None], p[None])                         # (B, H, W, 2)
    memory = maps.new_zeros((bs, c, H, W))
    for j in range(nsectors):
        s = _apply(_rot(j, nsectors), q)
        gx = (s[..., 0] - _f32((x_lo + mx) / 2)) / _f32((mx - x_lo) / 2)
        gy = (s[..., 1] - _f32((y_lo + my) / 2)) / _f32((my - y_lo) / 2)
        smp = F.grid_sample(maps[j * bs:(j + 1) * bs], torch.stack([gx, gy], -1), mode="bilinear", padding_mode="zeros", align_corners=False)
        memory = torch.where(smp.abs() > 0, smp, memory)
    return memory


def memory_read(memory: torch.Tensor, nsectors: int, pc_range=CART_RANGE) -> torch.Tensor:
    """memory (B, C, H, W) -> (nsectors * B, C, h, w), sector-major"""
    bs, c, H, W = memory.shape
    h, w = H // (2 if nsectors >= 2 else 1), W // (2 if nsectors >= 4 else 1)
    x_lo, y_lo, mx, my = _region(nsectors, pc_range)
    g = _corners(x_lo, y_lo, mx, my, h, w)
    out = []
    for j in range(nsectors):
        s = _apply(_rot(j, nsectors), g)
        grid = torch.stack([s[..., 0] / _f32((pc_range[3] - pc_range[0]) / 2), s[..., 1] / _f32((pc_range[4] - pc_range[1]) / 2)], -1)
        out.append(F.grid_sample(memory, grid[None].repeat(bs, 1, 1, 1), mode="bilinear", padding_mode="zeros", align_corners=False))
    return torch.cat(out)


# ------------------------------------------------------------------------------------------------------------------------ the reduced model
NSEC, BATCH, CLASSES, REL = 4, 2, 6, 1e-4
NECK = dict(layer_nums=[1, 1, 1], ds_layer_strides=[2, 2, 2], ds_num_filters=[32, 32, 64], us_layer_strides=[0.5, 1, 2], us_num_filters=[32, 32, 32],
            num_input_features=32)
TASKS = [dict(num_class=10, class_names=["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
                                         "traffic_cone"])]
TEST_CFG = dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], nms=dict(nms_pre_max_size=200, nms_post_max_size=40, nms_iou_threshold=0.2),
                score_threshold=0.02, pc_range=list(CART_RANGE), out_size_factor=4, voxel_size=list(CART_VOXEL[:2]), interval=NSEC, rectify=False,
                stateful_nms=True, panoptic=False)


def model_cfg(nsectors=NSEC, **over):
    """the reduced STROBE of strobe.npz as an inline config (the reference's strobe_4_sector.py at a 64 x 64 grid)"""
    import logging
    heads = {"reg": (2, 2), "rot_vel": (2, 2), "height": (1, 2), "dim": (3, 2)}
    cfg = dict(type="STROBE", nsectors=nsectors, pretrained=None,
               reader=dict(type="DynamicPFNet", num_filters=[32, 32], num_input_features=7, voxel_shape="cuboid", xyz_cluster=True, raz_cluster=True,
                           xy_center=True, ra_center=True, voxel_size=list(CART_VOXEL), pc_range=list(CART_RANGE)),
               backbone=dict(type="DynamicPPScatter", ds_factor=1),
               neck=dict(type="RPNUber", logger=logging.getLogger("RPN"), **NECK),
               bbox_head=dict(type="CenterHeadSingle", in_channels=96, tasks=TASKS, dataset="nuscenes", weight=0.5, code_weights=[1.0] * 10,
                              common_heads=heads, voxel_shape="cuboid"),
               seg_head=dict(type="SingleConvHead", num_classes=CLASSES, in_channels=128, kernel=1, loss=dict(type="SegLoss", ignore=-1)), part_head=None)
    cfg.update(over)
    return cfg


def stacked_example(g, k):
    """sweep k of strobe.npz as the collated example the reference's STROBE took (CPU tensors): the source rows are regenerated from
    their seeds, the columns the split rewrites and the cells are the reference's"""
    num = [int(v) for v in g[f"sw{k}_num"]]
    index, xyphi, cells = g[f"sw{k}_index"].astype(np.int64), g[f"sw{k}_xyphi"], g[f"sw{k}_cells"].astype(np.int64)
    src = [cuboid_sweep(n, seed) for seed, n in zip(SWEEP_SEEDS[k], SWEEP_POINTS)]
    cuts = np.concatenate([[0], np.cumsum(num)])
    rows = np.concatenate([src[p % BATCH][index[cuts[p]:cuts[p + 1]]] for p in range(NSEC * BATCH)])
    rows[:, [0, 1, 6]] = xyphi
    gi = np.concatenate([np.repeat(np.arange(NSEC * BATCH), num)[:, None], cells], 1)
    n = NSEC * BATCH
    return dict(points=torch.from_numpy(rows), grid_ind=torch.from_numpy(gi), num_points=num, voxel_size=np.stack([np.asarray(CART_VOXEL)] * n),
                pc_range=np.stack([np.asarray(CART_RANGE)] * n), grid_size=np.stack([np.asarray(sector_grid([64, 64, 1], NSEC))] * n),
                metadata=[dict(token=i % BATCH) for i in range(n)], valid_grid_ind=list(torch.split(torch.from_numpy(cells), num)),
                key_points_index=list(torch.split(torch.from_numpy(index), num)), transform_matrix=torch.cat([rotations(SWEEP_ANGLES[k], BATCH)] * NSEC))
