#!/usr/bin/env python3
"""Golden vectors of the seg super-task's loss: runs the REFERENCE's ``SegLoss`` (losses/seg_loss.py:8-22, lovasz_losses.py) and
``SingleConvHead.loss`` (seg_heads/seg_head.py:86-96), imported through ref_import.py, on deterministic inputs with its own autograd, and
stores the inputs and its fp32 outputs in ``seg_loss.npz``.

Container-only: ``python tests/golden/make_golden_seg_loss.py``.  Data only.
  (a) SegLoss(ignore=-1): case ``a16`` B = 2, C = 16, 24 x 40, logits N(0, 2^2), ~30 % of the cells labelled, class 11 absent, the first rows
      of sample 1 all ignored; case ``a6`` C = 6.  Per case: logits, labels, loss, d(loss)/d(logits).
  (b) SingleConvHead(kernel=1, num_classes=6, in_channels=20, weight=2).loss on x1 (2,12,24,40), x2 (2,8,6,10), voxel_labels (2,1,24,40):
      weights, inputs, seg_loss, the gradients w.r.t. weight, bias, x1, x2.
The generator asserts that no two errors of one class are equal (the reference's unstable torch.sort is then well defined) and that no
probability is exactly 0 or 1.
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
from det3d.models.losses.seg_loss import SegLoss  # noqa: E402
from det3d.models.seg_heads.seg_head import SingleConvHead  # noqa: E402

IGNORE = -1


def draw_labels(r, b, c, h, w, absent, frac=0.3, blank_rows=5):
    """(B,H,W) int64 in {-1, 0..c-1} \\ {absent}; ~frac of the cells labelled; the first ``blank_rows`` rows of sample 1 ignored"""
    classes = np.array([k for k in range(c) if k != absent])
    lab = classes[r.integers(0, len(classes), (b, h, w))]
    lab[r.uniform(0, 1, (b, h, w)) >= frac] = IGNORE
    lab[1, :blank_rows] = IGNORE
    return lab.astype(np.int64)


def check_well_defined(logits, labels):
    c = logits.shape[1]
    p = torch.softmax(torch.from_numpy(logits), 1).permute(0, 2, 3, 1).reshape(-1, c)
    lab = torch.from_numpy(labels).reshape(-1)
    vp, vl = p[lab != IGNORE], lab[lab != IGNORE]
    assert float(vp.min()) > 0.0 and float(vp.max()) < 1.0, "a probability is exactly 0 or 1"
    for k in range(c):
        err = ((vl == k).float() - vp[:, k]).abs()
        assert err.unique().numel() == err.numel(), f"class {k}: two equal errors"


def seg_loss_case(r, tag, b, c, h, w, absent, out):
    logits = (2.0 * r.standard_normal((b, c, h, w))).astype(np.float32)
    labels = draw_labels(r, b, c, h, w, absent)
    check_well_defined(logits, labels)
    x = torch.from_numpy(logits).clone().requires_grad_(True)
    loss = SegLoss(ignore=IGNORE)(x, torch.from_numpy(labels))
    loss.backward()
    out[f"{tag}_logits"], out[f"{tag}_labels"] = logits, labels
    out[f"{tag}_loss"], out[f"{tag}_grad"] = np.float32(loss.item()), x.grad.numpy()
    print(tag, "valid cells", int((labels != IGNORE).sum()), "classes present", len(np.unique(labels[labels != IGNORE])), "loss", loss.item())


def head_case(r, out):
    head = SingleConvHead(kernel=1, num_classes=6, in_channels=20, weight=2, loss=dict(type="SegLoss", ignore=IGNORE))
    with torch.no_grad():
        head.conv.weight.copy_(torch.from_numpy((0.4 * r.standard_normal((6, 20, 1, 1))).astype(np.float32)))
        head.conv.bias.copy_(torch.from_numpy((0.2 * r.standard_normal(6)).astype(np.float32)))
    x1 = torch.from_numpy(r.standard_normal((2, 12, 24, 40)).astype(np.float32)).requires_grad_(True)
    x2 = torch.from_numpy(r.standard_normal((2, 8, 6, 10)).astype(np.float32)).requires_grad_(True)
    voxel_labels = (draw_labels(r, 2, 6, 24, 40, absent=4) + 1)[:, None]                 # 0 = unlabelled
    preds = head(x1, x2)
    check_well_defined(preds["seg_preds"].detach().numpy(), voxel_labels[:, 0] - 1)
    seg_loss = head.loss(dict(voxel_labels=torch.from_numpy(voxel_labels)), preds)["seg_loss"][0]
    seg_loss.backward()
    out.update(h_weight=head.conv.weight.detach().numpy(), h_bias=head.conv.bias.detach().numpy(), h_x1=x1.detach().numpy(), h_x2=x2.detach().numpy(),
               h_voxel_labels=voxel_labels.astype(np.int64), h_seg_loss=np.float32(seg_loss.item()), h_grad_weight=head.conv.weight.grad.numpy(),
               h_grad_bias=head.conv.bias.grad.numpy(), h_grad_x1=x1.grad.numpy(), h_grad_x2=x2.grad.numpy(), h_head_weight=np.float32(2.0))
    print("head seg_loss", seg_loss.item())


def main():
    r = np.random.default_rng(11)
    out = dict(ignore=np.int64(IGNORE))
    seg_loss_case(r, "a16", 2, 16, 24, 40, 11, out)
    seg_loss_case(r, "a6", 2, 6, 10, 14, 3, out)
    head_case(r, out)
    path = os.path.join(HERE, "seg_loss.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote seg_loss.npz %8.1f KB" % (size / 1024))
    assert size < 400 * 1024


if __name__ == "__main__":
    main()
