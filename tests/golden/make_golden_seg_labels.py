#!/usr/bin/env python3
"""Golden vectors of the seg super-task's targets: runs the REFERENCE's ``Voxelization.get_grid_ind`` (datasets/pipelines/voxelization.py:
40-60) -- and thereby ``AssignLabel.assign_voxel_labels`` (datasets/pipelines/preprocess.py:170-191; numba's njit is the identity under
ref_import.py, so the loop runs as Python) -- and ``get_labels`` (models/seg_heads/seg_head.py:24-49), imported through ref_import.py, on
deterministic inputs and stores the inputs and its outputs in ``seg_labels.npz``.

Container-only: ``python tests/golden/make_golden_seg_labels.py``.  Data only.
  vote cases (per case ``{tag}_labels`` (N,) int64 point labels, -1 = unlabelled; ``{tag}_voxel_labels`` (B,Z,H,W) int64; grid_ind rows are
  [b, z, y, x]):
    small  the points / grid_ind of small_model.npz (B = 2, 64 x 64 x 1; grid_ind is read from there, not stored again), labels drawn from
           0..16 with ~10 % of the points at -1
    edge   a hand-built sweep on an 8 x 10 x 1 grid, B = 3, sample 1 empty: runs of 1, 63, 64, 65 and 3000 points, a two-label tie, a tie
           between 0 and k, a cell 0 wins outright, a cell of only -1 points, label 255, and a run whose first 64 points carry label A and
           whose later 70 points carry label B (a per-chunk winner would be wrong); ``edge_grid_ind`` (N,4) int64
    z3     Z = 3, H = 8, W = 10, B = 2, random; ``z3_grid_ind``
  pooled cases (``{tag}_labels`` in, ``{tag}_pred_shape``, ``{tag}_out`` int64): pool2d (2,12,21) -> (6,10), pool3to2 (2,3,12,20) -> (6,10),
  pool3to3 (2,4,12,20) -> (2,6,10); each holds windows with ties and windows of all-zero labels (asserted).
The reference is run per sample (a sample without labelled points is skipped: the reference indexes row 0 of an empty list).  The
generator asserts that no (cell, label) count reaches 65535, so the reference's uint16 counters never wrap.
"""
from __future__ import annotations

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
if not hasattr(np, "long"):          # numpy 2 dropped the alias the reference uses; this process only
    np.long = np.int64
from det3d.datasets.pipelines.voxelization import Voxelization  # noqa: E402
from det3d.models.seg_heads.seg_head import get_labels  # noqa: E402


def reference_vote(grid_ind, labels, batch, zhw):
    """(N,4) [b,z,y,x] + (N,) labels -> (B,Z,H,W) int64 by the reference, one sample at a time"""
    z, h, w = zhw
    vox = object.__new__(Voxelization)
    out = np.zeros((batch, z, h, w), np.int64)
    for b in range(batch):
        m = grid_ind[:, 0] == b
        if not (m & (labels >= 0)).any():
            continue
        res = dict(mode="train", lidar=dict(pc_label=labels[m].astype(np.int64)[:, None], voxels={}))
        vox.get_grid_ind(res, grid_ind[m, 1:].astype(np.int64), np.array([w, h, z]))
        out[b] = res["lidar"]["voxels"]["labels"][0]
    # the uint16 counters of the reference must not have wrapped
    ok = labels >= 0
    _, counts = np.unique(np.concatenate([grid_ind[ok], labels[ok, None]], 1), axis=0, return_counts=True)
    assert counts.max() < 65535
    return out


def edge_case(r):
    cells = []          # (b, y, x, labels in point order)

    def add(b, y, x, *groups):
        cells.append((b, y, x, np.concatenate([np.full(n, lab, np.int64) for lab, n in groups])))

    add(0, 0, 0, (5, 1))                                  # run of 1
    add(0, 0, 1, (3, 40), (7, 23))                        # 63
    add(0, 0, 2, (9, 32), (2, 32))                        # 64, two-label tie -> 2
    add(0, 1, 0, (4, 30), (8, 35))                        # 65
    add(0, 1, 1, (6, 1400), (12, 1500), (-1, 100))        # 3000
    add(0, 2, 3, (11, 5), (0, 5))                         # tie between 0 and 11 -> 0: unlabelled
    add(0, 3, 3, (-1, 7))                                 # only unlabelled points
    add(0, 7, 9, (16, 2), (-1, 3), (1, 2))                # tie 1 / 16 with unlabelled points between
    add(2, 7, 9, (255, 3), (1, 2))                        # label 255
    ab = len(cells)
    add(2, 4, 5, (13, 64), (14, 70))                      # 64 x A first, then 70 x B -> B
    add(2, 0, 0, (0, 4), (3, 1))                          # 0 wins outright
    add(2, 3, 0, (10, 1), (-1, 1))
    for _ in range(12):                                   # a few random cells in samples 0 and 2
        b, y, x = int(r.choice([0, 2])), int(r.integers(4, 7)), int(r.integers(0, 10))
        if any((b, y, x) == c[:3] for c in cells):
            continue
        n = int(r.integers(1, 9))
        lab = r.integers(0, 17, n)
        lab[r.uniform(0, 1, n) < 0.1] = -1
        cells.append((b, y, x, lab.astype(np.int64)))
    gi, lab, keep = [], [], []
    for k, (b, y, x, ls) in enumerate(cells):
        gi.append(np.tile(np.array([[b, 0, y, x]], np.int64), (len(ls), 1)))
        lab.append(ls)
        keep.append(np.full(len(ls), k))
    gi, lab, keep = np.concatenate(gi), np.concatenate(lab), np.concatenate(keep)
    # interleave the cells' points inside every sample; the A-then-B cell keeps its own order
    sort_key = r.uniform(0, 1, len(lab))
    idx = np.nonzero(keep == ab)[0]
    sort_key[idx] = np.sort(sort_key[idx])
    order = np.lexsort((sort_key, gi[:, 0]))
    gi, lab, keep = gi[order], lab[order], keep[order]
    run = lab[keep == ab]
    assert (run[:64] == 13).all() and (run[64:] == 14).all() and len(run) == 134
    return gi, lab


def pooled_case(r, shape, pred_shape):
    lab = r.choice(np.array([0, 0, 0, 1, 2, 3, 200, 255]), size=shape).astype(np.int64)
    lab[0, ..., :4, :6] = 0                                # windows of all-zero labels
    lab[1, ..., 4:6, 2:4] = np.array([[7, 9], [9, 7]])     # a tie inside one window (every plane, when there are planes)
    out = get_labels(torch.from_numpy(lab), tuple(pred_shape))
    return lab, out.numpy().astype(np.int64)


def main():
    r = np.random.default_rng(23)
    out = {}
    g = np.load(os.path.join(HERE, "small_model.npz"))
    gi = g["grid_ind"].astype(np.int64)
    lab = r.integers(0, 17, len(gi)).astype(np.int64)
    lab[r.uniform(0, 1, len(gi)) < 0.1] = -1
    out["small_labels"], out["small_voxel_labels"] = lab, reference_vote(gi, lab, 2, (1, 64, 64))

    gi, lab = edge_case(r)
    out["edge_grid_ind"], out["edge_labels"], out["edge_voxel_labels"] = gi, lab, reference_vote(gi, lab, 3, (1, 8, 10))
    vl = out["edge_voxel_labels"]
    assert vl[0, 0, 0, 2] == 2 and vl[0, 0, 1, 1] == 12 and vl[0, 0, 2, 3] == 0 and vl[0, 0, 3, 3] == 0 and vl[2, 0, 7, 9] == 255
    assert vl[2, 0, 4, 5] == 14 and vl[2, 0, 0, 0] == 0 and vl[0, 0, 7, 9] == 1 and not vl[1].any()

    n = 1500
    gi = np.stack([np.sort(r.integers(0, 2, n)), r.integers(0, 3, n), r.integers(0, 8, n), r.integers(0, 10, n)], 1).astype(np.int64)
    lab = r.integers(0, 21, n).astype(np.int64)
    lab[r.uniform(0, 1, n) < 0.1] = -1
    out["z3_grid_ind"], out["z3_labels"], out["z3_voxel_labels"] = gi, lab, reference_vote(gi, lab, 2, (3, 8, 10))

    for tag, shape, pred in (("pool2d", (2, 12, 21), (6, 10)), ("pool3to2", (2, 3, 12, 20), (6, 10)), ("pool3to3", (2, 4, 12, 20), (2, 6, 10))):
        lab, res = pooled_case(r, shape, pred)
        assert res.shape == (2,) + pred, res.shape
        assert (res == -1).any() and (res[1, ..., 2, 1] == 6).all()          # all-zero windows; the 7 / 9 tie goes to 7
        out[f"{tag}_labels"], out[f"{tag}_pred_shape"], out[f"{tag}_out"] = lab, np.array(pred, np.int64), res
        print(tag, lab.shape, "->", res.shape, "ignored windows", int((res == -1).sum()))

    path = os.path.join(HERE, "seg_labels.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote seg_labels.npz %8.1f KB" % (size / 1024))
    assert size < 400 * 1024


if __name__ == "__main__":
    main()
