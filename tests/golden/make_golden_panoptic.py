#!/usr/bin/env python3
"""Golden vectors of the panoptic fusion: runs the REFERENCE's ``SingleConvHead.predict_panoptic`` (seg_heads/seg_head.py:99-168,
imported through ref_import.py) on deterministic inputs and stores the inputs and its outputs in ``panoptic.npz``.

Container-only: ``python tests/golden/make_golden_panoptic.py``.  Data only: logits, grid indices, points, boxes with scores /
labels / instance ids, the class names and tokens, and the reference's per-point 'seg' / 'ins' for the cylinder runs (interval pi/2,
sector 0 and 3) and a cuboid run (interval 4, sector 1).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_import  # noqa: E402

det3d = ref_import.import_reference()
from addict import Dict as ADict  # stub from ref_import  # noqa: E402
from det3d.models.seg_heads.seg_head import SingleConvHead  # noqa: E402

CLASS_NAMES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]   # the config's order
TOKENS = ["a", "b"]
NUM_POINTS = [700, 513]
NUM_BOXES = 150
CLASSES, H, W = 16, 16, 12
INTERVAL_CYLINDER, INTERVAL_CUBOID = math.pi / 2, 4.0


def draw():
    r = np.random.default_rng(5)
    logits = r.standard_normal((2, CLASSES, H, W)).astype(np.float32)
    logits[:, :10] += np.float32(0.8)                       # most points carry a thing label
    out = dict(logits=logits)
    pts = []
    for b, n in enumerate(NUM_POINTS):
        p = r.standard_normal((n, 7)).astype(np.float32)
        p[:, 3:5] = r.uniform(-50, 50, (n, 2)).astype(np.float32)      # Cartesian x, y of a polar point row
        p[:, 0:2] = r.uniform(-50, 50, (n, 2)).astype(np.float32)      # read as x, y by the cuboid run
        pts.append(p)
        out[f"grid_ind{b}"] = np.stack([np.zeros(n, np.int64), r.integers(0, H, n), r.integers(0, W, n)], 1)
        boxes = r.standard_normal((NUM_BOXES, 9)).astype(np.float32)
        boxes[:, :2] = r.uniform(-50, 50, (NUM_BOXES, 2)).astype(np.float32)
        out[f"boxes{b}"] = boxes
        out[f"scores{b}"] = r.uniform(0, 1, NUM_BOXES).astype(np.float32)
        out[f"labels{b}"] = r.integers(0, 10, NUM_BOXES).astype(np.int64)
        out[f"instances{b}"] = (r.permutation(NUM_BOXES) + 1).astype(np.int64)
    out["points"] = np.concatenate(pts, 0)
    out["num_points"] = np.asarray(NUM_POINTS, np.int64)
    return out


def run_reference(d, voxel_shape, interval, sec_id):
    example = dict(num_points=torch.from_numpy(d["num_points"]), metadata=[dict(token=t) for t in TOKENS], points=torch.from_numpy(d["points"]),
                   valid_grid_ind=[torch.from_numpy(d[f"grid_ind{b}"]) for b in range(2)])
    det = [[dict(box3d_lidar=torch.from_numpy(d[f"boxes{b}"]), scores=torch.from_numpy(d[f"scores{b}"]), label_preds=torch.from_numpy(d[f"labels{b}"]),
                 instances=torch.from_numpy(d[f"instances{b}"])) for b in range(2)]]
    ret = SingleConvHead.predict_panoptic(None, example, dict(seg_preds=torch.from_numpy(d["logits"])), ADict(interval=interval), dict(det=det),
                                          voxel_shape=voxel_shape, class_names=[CLASS_NAMES], sec_id=sec_id)
    seg, ins = list(ret["seg"]), list(ret["ins"])
    return [seg[b][TOKENS[b]].numpy() for b in range(2)], [ins[b][TOKENS[b]].numpy() for b in range(2)]


def main():
    d = draw()
    out = dict(d, class_names=np.array(CLASS_NAMES), tokens=np.array(TOKENS), interval_cylinder=np.float64(INTERVAL_CYLINDER),
               interval_cuboid=np.float64(INTERVAL_CUBOID))
    for tag, shape, interval, sec in (("cyl0", "cylinder", INTERVAL_CYLINDER, 0), ("cyl3", "cylinder", INTERVAL_CYLINDER, 3), ("cub1", "cuboid", INTERVAL_CUBOID, 1)):
        seg, ins = run_reference(d, shape, interval, sec)
        for b in range(2):
            out[f"seg_{tag}_{b}"], out[f"ins_{tag}_{b}"] = seg[b].astype(np.int64), ins[b].astype(np.int64)
            print(tag, b, "thing points with an id:", int((ins[b] > 0).sum()), "of", len(ins[b]))
    path = os.path.join(HERE, "panoptic.npz")
    np.savez_compressed(path, **out)
    print("wrote panoptic.npz %8.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
