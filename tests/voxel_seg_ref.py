"""Restatement of the voxel-wise segmentation head (DeconvConvHead with height D > 1, det3d/models/seg_heads/seg_head.py:195-264), written
from the two formulas of DESIGN.md 4.4h and generic in the dtype: float64 is the reference of the GPU tests, the same functions in float32
give ``e32``, the error of the computation itself in f32.  Also the seeded inputs shared by tests/golden/make_golden_voxel_seg.py and the
tests (the 15.7 MB weight of the ``full_height`` case is drawn, not stored).

  u[b, Y, X, h]  = sum over the <= 2 x 2 pixels (iy, ix) with ky = Y + S/2 - S iy, kx = X + S/2 - S ix in [0, 2S):
                       sum_c x2[b, c, iy, ix] Wd[c, h, ky, kx]
  logit[b, c, z, y, x] = bias[c D + z] + sum_{dy, dx in {-1, 0, 1}, inside the map}
                       (  sum_{z' < D, k < 16} Wc[c D + z, k D + z', dy + 1, dx + 1] f1[b, k, z', y + dy, x + dx]
                        + sum_{h < D}          Wc[c D + z, 16 D + h, dy + 1, dx + 1] u[b, y + dy, x + dx, h]  )
"""
from __future__ import annotations

import numpy as np
import torch

CV = 16      # channels of the encoder's conv1 level

CASES = {
    # name: B, D, H, W, NC, Cin, up_scale, seed
    "small": dict(B=2, D=5, H=16, W=24, NC=6, Cin=12, S=8, seed=20240611),
    "full_height": dict(B=1, D=40, H=16, W=16, NC=16, Cin=24, S=8, seed=20240612),
}
OCCUPANCY = 0.08
N_INACTIVE = 200


def draw_case(name: str) -> dict:
    """the seeded weights and inputs of a case (float32 numpy): deconv_w (Cin, D, 2S, 2S), conv_w (NC D, 17 D, 3, 3), conv_b (NC D),
    x1 (B, 16, D, H, W) = conv1.dense() with about 8 % of the sites active (non-negative features, as behind a ReLU), x2 (B, Cin, H/S, W/S),
    inactive (200, 4) int64 cells [b, z, y, x] that hold no site.  Sample 1 of ``small`` is empty in its first 4 rows."""
    c = CASES[name]
    B, D, H, W, NC, Cin, S = (c[k] for k in ("B", "D", "H", "W", "NC", "Cin", "S"))
    g = np.random.Generator(np.random.PCG64(c["seed"]))
    f32 = np.float32
    deconv_w = (g.standard_normal((Cin, D, 2 * S, 2 * S)) / np.sqrt(Cin)).astype(f32)
    conv_w = (g.standard_normal((NC * D, (CV + 1) * D, 3, 3)) / np.sqrt(9.0 * D * (CV * OCCUPANCY + 1))).astype(f32)
    conv_b = (0.1 * g.standard_normal(NC * D)).astype(f32)
    mask = g.random((B, D, H, W)) < OCCUPANCY
    if name == "small":
        mask[1, :, :4, :] = False
    x1 = (np.abs(g.standard_normal((B, CV, D, H, W))) * mask[:, None]).astype(f32)
    x2 = g.standard_normal((B, Cin, H // S, W // S)).astype(f32)
    free = np.argwhere(~mask)
    inactive = free[np.sort(g.choice(len(free), N_INACTIVE, replace=False))].astype(np.int64)
    return dict(c, deconv_w=deconv_w, conv_w=conv_w, conv_b=conv_b, x1=x1, x2=x2, mask=mask, active=np.argwhere(mask).astype(np.int64),
                inactive=inactive)


def deconv(x2: torch.Tensor, wd: torch.Tensor, s: int) -> torch.Tensor:
    """x2 (B, Cin, h, w), wd (Cin, D, 2S, 2S) -> u (B, h S, w S, D), in the dtype of the inputs"""
    b, _, h, w = x2.shape
    d = wd.shape[1]
    u = torch.zeros((b, h * s, w * s, d), dtype=x2.dtype)
    for ky in range(2 * s):
        ys = [(iy, s * iy + ky - s // 2) for iy in range(h) if 0 <= s * iy + ky - s // 2 < h * s]
        for kx in range(2 * s):
            xs = [(ix, s * ix + kx - s // 2) for ix in range(w) if 0 <= s * ix + kx - s // 2 < w * s]
            if not ys or not xs:
                continue
            iy, yy = (torch.tensor(v) for v in zip(*ys))
            ix, xx = (torch.tensor(v) for v in zip(*xs))
            term = torch.einsum("bcij,ch->bijh", x2[:, :, iy][:, :, :, ix], wd[:, :, ky, kx])
            u[:, yy[:, None], xx[None, :]] += term
    return u


def logits_dense(x1: torch.Tensor, u: torch.Tensor, wc: torch.Tensor, bias: torch.Tensor, nc: int) -> torch.Tensor:
    """x1 (B, 16, D, H, W), u (B, H, W, D), wc (NC D, 17 D, 3, 3), bias (NC D) -> logits (B, NC, D, H, W) at every cell"""
    b, cv, d, h, w = x1.shape
    w6 = wc.reshape(nc, d, cv + 1, d, 3, 3)      # [c, z, k | dense, z' | h, ky, kx]
    out = bias.reshape(1, nc, d, 1, 1).expand(b, nc, d, h, w).clone()
    f1 = torch.nn.functional.pad(x1, (1, 1, 1, 1))
    up = torch.nn.functional.pad(u.permute(0, 3, 1, 2), (1, 1, 1, 1))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            f = f1[:, :, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            out = out + torch.einsum("czkq,bkqyx->bczyx", w6[:, :, :cv, :, dy + 1, dx + 1], f)
            out = out + torch.einsum("czq,bqyx->bczyx", w6[:, :, cv, :, dy + 1, dx + 1], up[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
    return out


def head_dense(case: dict, dtype=torch.float64):
    """(u, logits at every cell) of a drawn case in ``dtype``"""
    t = lambda k: torch.from_numpy(case[k]).to(dtype)  # noqa: E731
    u = deconv(t("x2"), t("deconv_w"), case["S"])
    return u, logits_dense(t("x1"), u, t("conv_w"), t("conv_b"), case["NC"])


def at_cells(dense: torch.Tensor, cells) -> torch.Tensor:
    """dense (B, NC, D, H, W), cells (n, 4) [b, z, y, x] -> (n, NC)"""
    c = torch.as_tensor(np.asarray(cells)).long()
    return dense[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]


def cell_keys(cells, d, h, w) -> np.ndarray:
    c = np.asarray(cells).astype(np.int64)
    return (((c[:, 0] * d + c[:, 1]) * h + c[:, 2]) * w + c[:, 3]).astype(np.int32)


def labels_and_gap(rows: torch.Tensor):
    """rows (n, NC) float64 -> (1 + argmax (lowest among equals), the gap between the two largest logits)"""
    top = torch.topk(rows, 2, dim=1).values
    best = rows.max(1, keepdim=True).values
    first = (rows == best).to(torch.int64).argmax(1)      # the first maximal class
    return first + 1, top[:, 0] - top[:, 1]
