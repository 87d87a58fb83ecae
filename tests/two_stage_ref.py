"""Shared by tests/golden/make_golden_two_stage.py and the two-stage tests: the seeded inputs of the golden cases (only what the
reference computes is stored in two_stage.npz) and a torch-CPU restatement of the whole second stage, written from the description in
include/partner_hip.h (pn_roi_bev_gather_f32, pn_roi_refine_f32) and the layer list of the RoIHead -- not from the reference's code.

Everything is float32 torch on the CPU; the restatement keeps the order of operations the header names (two divisions, floor, clamp,
weights from the clamped indices, the four products summed left to right)."""
from __future__ import annotations

import math

import numpy as np
import torch

REL = 1e-4                     # the project's bound for f32 paths against the reference, of max |ref| per compared tensor

PC_START = (-8.0, -6.0)
VOXEL_SIZE = (0.2, 0.25)
OUT_STRIDE = 2                 # cells of 0.4 x 0.5: a 40 x 24 map spans x in [-8, 8), y in [-6, 6)

# tag: B, H, W, C, num_point, box columns, counts, cap_in, max_rois, seed
GATHER_CASES = {
    "A": dict(batch=2, h=24, w=40, c=20, num_point=5, cols=7, counts=(7, 0), cap_in=12, max_rois=12, seed=101),
    "B": dict(batch=2, h=24, w=40, c=64, num_point=1, cols=9, counts=(5, 12), cap_in=12, max_rois=16, seed=202),
}

# x, y, z, d0, d1, d2, rotation: all four quadrants of the rotation; a face midpoint left of, right of, below and above the map; a centre outside
CRAFTED = (
    (0.33, 0.21, -0.5, 1.8, 4.2, 1.6, 0.4),
    (-7.47, 1.13, 0.2, 2.0, 4.5, 1.7, 2.0),       # a side midpoint left of column 0
    (7.03, -2.31, 0.1, 1.6, 3.8, 1.5, -2.5),      # right of column W - 1
    (1.71, 5.03, -0.3, 2.2, 4.0, 1.4, -0.7),      # below row H - 1
    (-2.23, -5.31, 0.4, 1.9, 4.4, 1.8, 1.2),      # above row 0
    (8.93, 0.41, 0.0, 1.5, 3.5, 1.5, 3.0),        # the centre itself right of the map
    (-3.37, 2.77, -0.1, 0.9, 0.8, 1.7, -1.9),
)

HEAD_CFG = dict(SHARED_FC=[64, 32], CLS_FC=[32, 16], REG_FC=[16, 32], DP_RATIO=0.3)
HEAD_ROWS, HEAD_CHANNELS, HEAD_SEED = 24, 100, 31
REFINE_CASES = {7: "A", 9: "B"}      # code_size -> the gather case whose ROI buffers the refinement runs on


def gather_inputs(tag):
    """-> boxes (B, cap_in, cols), scores (B, cap_in), labels (B, cap_in) int64, counts (B,) int32, bev (B, H, W, C); rows at or past the
    count are NaN / -1 (never to be read)"""
    k = GATHER_CASES[tag]
    r = np.random.default_rng(k["seed"])
    b, cap, cols = k["batch"], k["cap_in"], k["cols"]
    boxes = np.full((b, cap, cols), np.nan, np.float32)
    scores = np.full((b, cap), np.nan, np.float32)
    labels = np.full((b, cap), -1, np.int64)
    for i, n in enumerate(k["counts"]):
        rows = [list(c) for c in CRAFTED[:n]]
        for _ in range(n - len(rows)):      # seeded boxes over a region a little wider than the map
            rows.append([r.uniform(-9.0, 9.0), r.uniform(-7.0, 7.0), r.uniform(-1, 1), r.uniform(0.6, 2.4), r.uniform(0.6, 5.0), r.uniform(1, 2),
                         r.uniform(-math.pi, math.pi)])
        rows = np.asarray(rows, np.float32).reshape(n, 7)
        if cols == 9:                       # the head's order: [x, y, z, w, l, h, vx, vy, rot]
            rows = np.concatenate([rows[:, :6], r.uniform(-3, 3, (n, 2)).astype(np.float32), rows[:, 6:]], 1)
        boxes[i, :n] = rows
        scores[i, :n] = r.uniform(0.1, 1.0, n).astype(np.float32)
        labels[i, :n] = r.integers(0, 3, n)
    bev = r.standard_normal((b, k["h"], k["w"], k["c"])).astype(np.float32)
    return (torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(labels), torch.tensor(k["counts"], dtype=torch.int32),
            torch.from_numpy(bev))


def head_features():
    return torch.from_numpy(np.random.default_rng(HEAD_SEED).standard_normal((HEAD_ROWS, HEAD_CHANNELS)).astype(np.float32))


def refine_inputs(code_size):
    """the seeded raw RoIHead outputs of a refine case -> rcnn_cls (B * max_rois, 1), rcnn_reg (B * max_rois, code_size)"""
    k = GATHER_CASES[REFINE_CASES[code_size]]
    r = np.random.default_rng(700 + code_size)
    rows = k["batch"] * k["max_rois"]
    return (torch.from_numpy(r.standard_normal((rows, 1)).astype(np.float32) * 2),
            torch.from_numpy(r.standard_normal((rows, code_size)).astype(np.float32) * 0.5))


# ------------------------------------------------------------------------------------------------ the restatement
def box_points(boxes: torch.Tensor, num_point: int) -> torch.Tensor:
    """(n, 7|9) boxes -> (n, num_point, 2): the centre, then the front, back, left and right face midpoints.  The rotation is the LAST
    column, the dims are columns 3:5; corner k = dims * sign_k rotated by (x cos + y sin, -x sin + y cos) + the centre; a midpoint is
    (corner + corner) / 2 with front = 0, 1; back = 2, 3; left = 0, 3; right = 1, 2"""
    pts = [boxes[:, :2]]
    if num_point == 5:
        s, c = torch.sin(boxes[:, -1]), torch.cos(boxes[:, -1])
        corners = []
        for sx, sy in ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5)):
            lx, ly = boxes[:, 3] * sx, boxes[:, 4] * sy
            corners.append(torch.stack([(lx * c + ly * s) + boxes[:, 0], (lx * (-s) + ly * c) + boxes[:, 1]], 1))
        for i, j in ((0, 1), (2, 3), (0, 3), (1, 2)):
            pts.append((corners[i] + corners[j]) / 2)
    else:
        assert num_point == 1
    return torch.stack(pts, 1)


def cells_of(points: torch.Tensor, pc_start=PC_START, voxel_size=VOXEL_SIZE, out_stride=OUT_STRIDE):
    """(.., 2) points -> the map coordinates x, y: (a - start) / voxel / out_stride, two divisions"""
    return ((points[..., 0] - pc_start[0]) / voxel_size[0] / out_stride, (points[..., 1] - pc_start[1]) / voxel_size[1] / out_stride)


def sample_map(im: torch.Tensor, x: torch.Tensor, y: torch.Tensor, magnitude=False) -> torch.Tensor:
    """(H, W, C) map, (n,) coordinates -> (n, C): floor, the four indices clamped to the map, the weights formed from the CLAMPED indices;
    in the dtype of its arguments.  ``magnitude``: the sum of the four products' absolute values (the scale of what cancels when a
    point lies outside the map)"""
    h, w = im.shape[:2]
    f = lambda i: i.to(x.dtype)      # noqa: E731
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    x1, y1 = (x0 + 1).clamp(0, w - 1), (y0 + 1).clamp(0, h - 1)
    x0, y0 = x0.clamp(0, w - 1), y0.clamp(0, h - 1)
    wa, wb = (f(x1) - x) * (f(y1) - y), (f(x1) - x) * (y - f(y0))
    wc, wd = (x - f(x0)) * (f(y1) - y), (x - f(x0)) * (y - f(y0))
    ta, tb, tc, td = im[y0, x0] * wa[:, None], im[y1, x0] * wb[:, None], im[y0, x1] * wc[:, None], im[y1, x1] * wd[:, None]
    if magnitude:
        ta, tb, tc, td = ta.abs(), tb.abs(), tc.abs(), td.abs()
    return ((ta + tb) + tc) + td


def gather(boxes, scores, labels, counts, bev, num_point, code_size, max_rois, pc_start=PC_START, voxel_size=VOXEL_SIZE, out_stride=OUT_STRIDE,
           magnitude=False):
    """pn_roi_bev_gather_f32 -> rois (B, max_rois, code_size), roi_scores, roi_labels (int64, label + 1), roi_features (B, max_rois, P * C),
    evaluated in the dtype of ``boxes`` and ``bev`` (float32 as the kernel, or float64)"""
    b, _, cols = boxes.shape
    c, dt = bev.shape[-1], boxes.dtype
    assert cols == code_size and bev.dtype == dt
    rois, rs = torch.zeros((b, max_rois, code_size), dtype=dt), torch.zeros((b, max_rois), dtype=scores.dtype)
    rl, feat = torch.zeros((b, max_rois), dtype=torch.int64), torch.zeros((b, max_rois, num_point * c), dtype=dt)
    for i in range(b):
        n = int(counts[i])
        if n == 0:
            continue
        bx = boxes[i, :n]
        rois[i, :n] = bx[:, [0, 1, 2, 3, 4, 5, 8, 6, 7]] if code_size == 9 else bx
        rs[i, :n], rl[i, :n] = scores[i, :n], labels[i, :n] + 1
        x, y = cells_of(box_points(bx, num_point), pc_start, voxel_size, out_stride)      # (n, P)
        feat[i, :n] = sample_map(bev[i], x.reshape(-1), y.reshape(-1), magnitude).reshape(n, num_point * c)
    return rois, rs, rl, feat


def roi_head_rows(sd, feats: torch.Tensor, prefix=""):
    """the RoIHead's layers on (rows, channels) features from its state_dict: every Conv1d(k = 1) + eval BatchNorm1d + ReLU of
    shared_fc_layer, then of cls_layers / reg_layers, then each branch's biased Conv1d -> rcnn_cls (rows, 1), rcnn_reg (rows, code_size)"""
    def run(name, x):
        idx = sorted({int(k[len(prefix + name) + 1:].split(".")[0]) for k in sd if k.startswith(prefix + name + ".") and k.endswith(".weight")})
        for i in idx:
            w = sd[f"{prefix}{name}.{i}.weight"].float()
            if w.dim() == 3:          # a convolution
                x = x @ w[:, :, 0].t()
                if f"{prefix}{name}.{i}.bias" in sd:
                    x = x + sd[f"{prefix}{name}.{i}.bias"].float()
            else:                     # its BatchNorm1d (eps 1e-5), then the ReLU
                p = f"{prefix}{name}.{i}."
                x = (x - sd[p + "running_mean"]) / torch.sqrt(sd[p + "running_var"] + 1e-5) * w + sd[p + "bias"]
                x = torch.relu(x)
        return x
    shared = run("shared_fc_layer", feats)
    return run("cls_layers", shared), run("reg_layers", shared)


def refine(rois, roi_scores, roi_labels, counts, rcnn_cls, rcnn_reg):
    """pn_roi_refine_f32 -> boxes (B, max_rois, code_size) in the head's order, scores, labels, counts; rows at or past the count zero
    (whatever the inputs hold there).  Evaluated in the dtype of its arguments"""
    b, r, cs = rois.shape
    reg, cls = rcnn_reg.reshape(b, r, cs), rcnn_cls.reshape(b, r)
    s, c = torch.sin(rois[..., 6]), torch.cos(rois[..., 6])
    out = reg + rois
    out[..., 0] = (reg[..., 0] * c + reg[..., 1] * s) + rois[..., 0]
    out[..., 1] = (reg[..., 0] * (-s) + reg[..., 1] * c) + rois[..., 1]
    if cs == 9:
        out = out[..., [0, 1, 2, 3, 4, 5, 7, 8, 6]]
    scores = torch.sqrt(torch.sigmoid(cls) * roi_scores)
    labels = roi_labels - 1
    live = torch.arange(r)[None, :] < counts.long()[:, None]
    return (torch.where(live[..., None], out, torch.zeros_like(out)), torch.where(live, scores, torch.zeros_like(scores)),
            torch.where(live, labels, torch.zeros_like(labels)), counts.clone())


def second_stage(sd, dets, bev, num_point, code_size, max_rois, pc_start, voxel_size, out_stride, prefix="roi_head."):
    """the whole second stage on a first stage's device list (CPU copies) and its NHWC neck output"""
    rois, rs, rl, feat = gather(dets["box3d_lidar"], dets["scores"], dets["label_preds"], dets["count"], bev, num_point, code_size, max_rois,
                                pc_start, voxel_size, out_stride)
    cls, reg = roi_head_rows(sd, feat.reshape(-1, feat.shape[-1]), prefix)
    return refine(rois, rs, rl, dets["count"], cls, reg)
