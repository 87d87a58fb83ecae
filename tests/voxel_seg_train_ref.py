"""Reference of the voxel segmentation head's TRAINING path, shared by tests/test_voxel_seg_train_cpu.py, tests/test_hip_voxel_seg_train.py
and tests/golden/make_golden_voxel_seg_train.py: seeded voxel labels for the two cases of tests/voxel_seg_ref.py and autograd (float64:
the reference; float32: ``e32``, the error of the computation itself) through ``R.deconv`` -> ``R.logits_dense`` -> the rows at the
labelled cells -> the SegLoss of tests/seg_loss_ref.py.

The labels: most of the active cells of every sample but the last of a batch of two (which has NO label at all), 40 cells that hold no
site, cells on the map border (y = 0, x = W - 1, z = 0, z = D - 1), one cell labelled NC + 1 (ignored) and zeros elsewhere (ignored)."""
from __future__ import annotations

import numpy as np
import torch

from tests import voxel_seg_ref as R
from tests.seg_loss_ref import seg_loss_terms


def draw_labels(case: dict, seed: int = 5) -> np.ndarray:
    """-> voxel_labels (B, D, H, W) uint8, 0 = unlabelled"""
    B, D, H, W, NC = (case[k] for k in ("B", "D", "H", "W", "NC"))
    g = np.random.Generator(np.random.PCG64(case["seed"] + seed))
    lab = np.zeros((B, D, H, W), np.uint8)
    nb = B - 1 if B > 1 else 1      # the samples that carry labels
    act = case["active"][case["active"][:, 0] < nb]
    act = act[g.random(len(act)) < 0.8]
    ina = case["inactive"][case["inactive"][:, 0] < nb][:40]
    border = np.array([[0, D // 2, 0, 3], [0, D // 2, 5, W - 1], [0, 0, 7, 7], [0, D - 1, 9, 2], [0, 0, 0, 0], [0, D - 1, H - 1, W - 1]])
    cells = np.concatenate([act, ina, border], 0)
    lab[cells[:, 0], cells[:, 1], cells[:, 2], cells[:, 3]] = g.integers(1, NC + 1, len(cells)).astype(np.uint8)
    lab[0, D // 2, H // 2, W // 2] = NC + 1      # above NC: ignored
    lab[0, D // 2, H // 2, W // 2 + 1] = 0       # a zero in the middle of the map: ignored
    assert (lab[nb:] == 0).all() or B == 1
    return lab


def labelled_cells(lab: np.ndarray, nc: int):
    """-> (cells (n, 4) in key order, labels - 1 (n,))"""
    flat = lab.reshape(-1)
    idx = np.flatnonzero((flat >= 1) & (flat <= nc))
    return np.stack(np.unravel_index(idx, lab.shape), 1).astype(np.int64), flat[idx].astype(np.int64) - 1


def leaves(case: dict, dtype):
    """the five differentiable inputs of the head as leaf tensors"""
    return {k: torch.from_numpy(case[k]).to(dtype).clone().requires_grad_(True) for k in ("deconv_w", "conv_w", "conv_b", "x2", "x1")}


def rows_at(case: dict, lv: dict, cells):
    """the head's logits rows (n, NC) at ``cells`` and the up-sampled map, differentiable"""
    u = R.deconv(lv["x2"], lv["deconv_w"], case["S"])
    u.retain_grad()
    dense = R.logits_dense(lv["x1"], u, lv["conv_w"], lv["conv_b"], case["NC"])
    return R.at_cells(dense, cells), u


def head_loss(case: dict, lab: np.ndarray, dtype, weight: float = 1.0) -> dict:
    """``weight * SegLoss(ignore=-1)`` over the labelled cells and its gradients
    -> dict(loss, rows, deconv_w, conv_w, conv_b, x2 (B, Cin, h, w), x1_rows (active, 16), u (B, H, W, D), errors: per class |fg - p|)"""
    cells, targets = labelled_cells(lab, case["NC"])
    lv = leaves(case, dtype)
    rows, u = rows_at(case, lv, cells)
    n, nc = rows.shape
    loss = weight * seg_loss_terms(rows.t().reshape(1, nc, n, 1), torch.from_numpy(targets).view(1, n, 1), -1)[0]
    loss.backward()
    a = case["active"]
    p = torch.softmax(rows.detach(), 1)
    fg = torch.nn.functional.one_hot(torch.from_numpy(targets), nc).to(p.dtype)
    out = {k: v.grad.detach() for k, v in lv.items() if k != "x1"}
    out.update(loss=float(loss.detach()), rows=rows.detach(), x1_rows=lv["x1"].grad[a[:, 0], :, a[:, 1], a[:, 2], a[:, 3]].detach(), u=u.grad.detach(),
               errors=(fg - p).abs(), targets=targets, cells=cells)
    return out


def no_equal_errors(errors: torch.Tensor, targets) -> bool:
    """no two equal Lovasz errors within a present class (float64): the sort's tie order is then irrelevant"""
    present = np.unique(targets)
    return all(len(torch.unique(errors[:, int(c)])) == errors.shape[0] for c in present)


def rows_backward(case: dict, cells, g_rows: np.ndarray, dtype) -> dict:
    """gradients of sum(rows * g_rows) -- the backward of the logits at ``cells`` alone, for a drawn ``g_rows`` (n, NC)
    -> dict(conv_w, conv_b, x1_rows, u)"""
    lv = leaves(case, dtype)
    rows, u = rows_at(case, lv, cells)
    if len(cells):
        (rows * torch.from_numpy(g_rows).to(dtype)).sum().backward()
    a = case["active"]
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad.detach()  # noqa: E731
    return dict(conv_w=z(lv["conv_w"]), conv_b=z(lv["conv_b"]), x1_rows=z(lv["x1"])[a[:, 0], :, a[:, 1], a[:, 2], a[:, 3]],
                u=torch.zeros_like(u) if u.grad is None else u.grad.detach())
