#!/usr/bin/env python3
"""Golden vectors of the voxel-wise segmentation head: runs the REFERENCE's ``DeconvConvHead`` (seg_heads/seg_head.py:223-264, imported
through ref_import.py) in eval mode on the CPU in f32, on the seeded inputs of tests/voxel_seg_ref.py, and stores data only in
``voxel_seg.npz``.

Container-only: ``python tests/golden/make_golden_voxel_seg.py``.
  small        B 2, D 5, 16 x 24, NC 6, Cin 12: weights, inputs and the reference's logits at every cell
  full_height  B 1, D 40, 16 x 16, NC 16, Cin 24: the seed, the inputs (x1 as active cells + feature rows, x2), the cells and the
               reference's logits at the active cells plus 200 seeded inactive cells -- the weights are drawn again by the tests
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
from det3d.models.seg_heads.seg_head import DeconvConvHead  # noqa: E402

from tests import voxel_seg_ref as R  # noqa: E402


def run_reference(case):
    head = DeconvConvHead(kernel=3, num_classes=case["NC"], in_channels_voxel=R.CV, in_channels=case["Cin"], up_scale=case["S"], height=case["D"],
                          loss=dict(type="SegLoss", ignore=-1))      # the reference cannot be built without a loss
    head.eval()
    with torch.no_grad():
        head.deconv.weight.copy_(torch.from_numpy(case["deconv_w"]))
        head.conv.weight.copy_(torch.from_numpy(case["conv_w"]))
        head.conv.bias.copy_(torch.from_numpy(case["conv_b"]))
        out = head(torch.from_numpy(case["x1"]), torch.from_numpy(case["x2"]))["seg_preds"]
    assert out.dtype == torch.float32 and tuple(out.shape) == (case["B"], case["NC"], case["D"], case["H"], case["W"])
    return out


def main():
    out = {}
    for name in R.CASES:
        case = R.draw_case(name)
        ref = run_reference(case)
        occ = case["mask"].mean()
        print(f"{name}: occupancy {occ:.3f}, {len(case['active'])} active cells, max |logit| {float(ref.abs().max()):.3f}")
        out[f"{name}_seed"] = np.int64(case["seed"])
        out[f"{name}_x2"] = case["x2"]
        out[f"{name}_active"] = case["active"]
        out[f"{name}_inactive"] = case["inactive"]
        a = case["active"]
        out[f"{name}_x1_rows"] = case["x1"][a[:, 0], :, a[:, 1], a[:, 2], a[:, 3]]
        if name == "small":
            for k in ("deconv_w", "conv_w", "conv_b"):
                out[f"{name}_{k}"] = case[k]
            out[f"{name}_logits"] = ref.numpy()
        else:
            cells = np.concatenate([case["active"], case["inactive"]], 0)
            out[f"{name}_cells"] = cells
            out[f"{name}_logits_at_cells"] = R.at_cells(ref, cells).numpy()
    path = os.path.join(HERE, "voxel_seg.npz")
    np.savez_compressed(path, **out)
    print("wrote voxel_seg.npz %8.1f KB" % (os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
