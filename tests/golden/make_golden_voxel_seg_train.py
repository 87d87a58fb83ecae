#!/usr/bin/env python3
"""Golden vectors of the voxel-wise segmentation head's TRAINING path: runs the REFERENCE's ``DeconvConvHead`` (seg_heads/seg_head.py:223-264,
imported through ref_import.py) in train mode on the CPU in f32 -- ``forward``, ``loss`` (seg_head.py:86-96: ``get_labels`` + ``weight *
SegLoss(ignore=-1)``) and autograd -- on the ``small`` case of tests/voxel_seg_ref.py with the seeded labels of
tests/voxel_seg_train_ref.py, and stores data only in ``voxel_seg_train.npz``: the labels, the loss and the gradients of the three
parameters, of x2 and of x1 at its active sites.

Container-only: ``python tests/golden/make_golden_voxel_seg_train.py``."""
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
from tests import voxel_seg_train_ref as T  # noqa: E402

WEIGHT = 2


def main():
    case = R.draw_case("small")
    lab = T.draw_labels(case)
    head = DeconvConvHead(kernel=3, num_classes=case["NC"], in_channels_voxel=R.CV, in_channels=case["Cin"], up_scale=case["S"], height=case["D"],
                          weight=WEIGHT, loss=dict(type="SegLoss", ignore=-1))
    head.train()
    with torch.no_grad():
        head.deconv.weight.copy_(torch.from_numpy(case["deconv_w"]))
        head.conv.weight.copy_(torch.from_numpy(case["conv_w"]))
        head.conv.bias.copy_(torch.from_numpy(case["conv_b"]))
    x1 = torch.from_numpy(case["x1"]).clone().requires_grad_(True)
    x2 = torch.from_numpy(case["x2"]).clone().requires_grad_(True)
    preds = head(x1, x2)
    # the reference's cross entropy raises on a label above NC ("Target 6 is out of bounds"); the port ignores such a cell, which is what
    # the reference computes with the cell unlabelled -- the stored labels keep it
    seen = np.where(lab > case["NC"], 0, lab).astype(np.int64)
    example = dict(voxel_labels=torch.from_numpy(seen).unsqueeze(1))
    loss = head.loss(example, preds)["seg_loss"][0]
    loss.backward()
    a = case["active"]
    out = dict(seed=np.int64(case["seed"]), weight=np.int64(WEIGHT), voxel_labels=lab, loss=np.float32(loss.item()),
               grad_deconv_w=head.deconv.weight.grad.numpy(), grad_conv_w=head.conv.weight.grad.numpy(), grad_conv_b=head.conv.bias.grad.numpy(),
               grad_x2=x2.grad.numpy(), grad_x1_rows=x1.grad.numpy()[a[:, 0], :, a[:, 1], a[:, 2], a[:, 3]])
    print(f"small: {int(((lab >= 1) & (lab <= case['NC'])).sum())} labelled cells, loss {loss.item():.6f}")
    path = os.path.join(HERE, "voxel_seg_train.npz")
    np.savez_compressed(path, **out)
    print("wrote voxel_seg_train.npz %8.1f KB" % (os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
