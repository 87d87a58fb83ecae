"""Shared by tests/golden/make_golden_two_stage_train.py and the two-stage training tests: the seeded inputs of the golden cases (only what
the reference computes is stored in two_stage_train.npz) and a torch-CPU restatement of the proposal targets and the RoIHead's loss, written
from the description in include/partner_hip.h (pn_roi_max_iou3d_f32, pn_roi_sample_targets_f32, pn_roi_loss_f32) -- not from the
reference's code.  The 3-D IoU is oracle.e2e_loss_oracle.iou3d_pairs (the restatement of boxes_iou3d_gpu the README lists as unpinned).

Sizes: B = 3 samples, R = 24 ROI slots, N = 12 gt rows, M = 16 sampled rows, F = HEAD_CHANNELS features; the thresholds are the
reference configs' own.  Crafted content (asserted by the generator): sample 0 has more foreground ROIs than round(0.5 M), hard and easy
background with n_hard < int(bg_needed * 0.8), and padding slots; sample 1 has fewer foreground ROIs than the quota, an ROI whose best gt
is of another class, an ROI equal to its gt, one with full BEV and partial height overlap, one rotated by pi / 2 on the same footprint,
rotations in all four quadrants and a yaw difference that takes the opposite-orientation flip; sample 2 has no gt.  Case "fgonly": one
sample of R foreground ROIs taken from sample 0 (the np.random.rand branch)."""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import two_stage_ref as TR2

REL = TR2.REL
B, R, N, M, F = 3, 24, 12, 16, TR2.HEAD_CHANNELS
HEAD_CFG = dict(TR2.HEAD_CFG, DP_RATIO=0)
HEAD_SEED = 53
TARGET_CFG = dict(ROI_PER_IMAGE=M, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25,
                  CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
LOSS_CFG = dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="L1",
                LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]))
THRESHOLDS = (0.1, 0.25, 0.55, 0.75)
MARGIN = 1e-2
COUNTS = (20, 14, 10)
# (by_class, score_type, code_size) of the stored target cases
CASES = ((True, "roi_iou", 7), (False, "roi_iou", 7), (True, "cls", 7), (False, "cls", 7), (True, "roi_iou", 9), (True, "cls", 9))


def case_name(by_class, score_type, cs, fgonly=False):
    return f"{'fgonly' if fgonly else 'main'}_{'bycls' if by_class else 'all'}_{score_type}_{cs}"


def target_cfg(by_class=True, score_type="roi_iou"):
    return dict(TARGET_CFG, SAMPLE_ROI_BY_EACH_CLASS=bool(by_class), CLS_SCORE_TYPE=score_type)


def code_weights(cs):
    return LOSS_CFG["LOSS_WEIGHTS"]["code_weights"][:cs]


def loss_cfg(cs):
    """LOSS_CFG with the code weights of a ``cs``-column head"""
    return dict(LOSS_CFG, LOSS_WEIGHTS=dict(LOSS_CFG["LOSS_WEIGHTS"], code_weights=code_weights(cs)))


# ------------------------------------------------------------------------------------------------ inputs
def _moved(g, r, shift, dz=0.0, drot=0.0):
    """a gt row [x, y, z, w, l, h, rot] moved by `shift` of its (w, l) along its own axes, dz of its height and drot"""
    c, s = math.cos(g[6]), math.sin(g[6])
    ax, ay = shift * g[3] * r.choice([-1, 1]), shift * g[4] * r.choice([-1, 1]) * 0.5
    return [g[0] + ax * c - ay * s, g[1] + ax * s + ay * c, g[2] + dz * g[5], g[3] * r.uniform(0.97, 1.03), g[4] * r.uniform(0.97, 1.03),
            g[5] * r.uniform(0.97, 1.03), g[6] + drot]


def _inputs7():
    """-> rois (B, R, 7), labels (B, R) int64, scores (B, R), gt (B, N, 8) as float64 lists turned float32"""
    r = np.random.default_rng(20240613)
    rois, labels, gt = np.zeros((B, R, 7)), np.zeros((B, R), np.int64), np.zeros((B, N, 8))
    # sample 0: six gts on a 3 x 2 grid, rotations spread; 10 fg, 3 hard, 7 easy ROIs, 4 padding slots
    g0 = []
    for k in range(6):
        g0.append([-12.0 + 12.0 * (k % 3) + r.uniform(-1, 1), -8.0 + 16.0 * (k // 3) + r.uniform(-1, 1), r.uniform(-0.5, 0.5), r.uniform(1.8, 2.2),
                   r.uniform(4.0, 4.8), r.uniform(1.5, 1.8), r.uniform(-math.pi, math.pi), 1 + k % 3])
    gt[0, :6] = g0
    rows, labs = [], []
    for k in range(10):
        g = g0[k % 6]
        rows.append(_moved(g, r, 0.06 + 0.02 * (k // 6), drot=r.uniform(-0.03, 0.03)))
        labs.append(g[7])
    for k in range(3):
        g = g0[k]
        rows.append(_moved(g, r, 0.42 + 0.06 * k))
        labs.append(g[7])
    for k in range(7):
        rows.append([r.uniform(-30, 30), 30.0 + 6.0 * k, r.uniform(-0.5, 0.5), 2.0, 4.4, 1.6, r.uniform(-math.pi, math.pi)])
        labs.append(1 + k % 3)
    order = r.permutation(COUNTS[0])            # the lists are no runs of neighbouring slots
    rois[0, :COUNTS[0]], labels[0, :COUNTS[0]] = np.asarray(rows)[order], np.asarray(labs)[order]

    # sample 1: crafted ROIs
    g1 = [[3.0, 2.0, 0.2, 2.0, 4.4, 1.6, 0.5, 1],             # quadrant 1
          [-9.0, 6.5, -0.3, 1.9, 4.1, 1.7, 2.2, 2],           # quadrant 2
          [-14.0, -9.0, 0.1, 2.1, 4.6, 1.5, -2.4, 3],         # quadrant 3
          [12.0, -7.0, 0.0, 2.2, 4.3, 1.8, -0.8, 1],          # quadrant 4
          [20.0, 10.0, 0.3, 2.0, 4.0, 1.6, 1.1, 2],           # the gt the class-1 ROI below overlaps best ...
          [20.5, 11.3, 0.3, 2.0, 4.0, 1.6, 1.1, 1]]           # ... and the class-1 gt it overlaps less
    gt[1, :6] = g1
    c1 = [list(g1[0][:7]),                                                                   # 0: equal to its gt (IoU 1)
          g1[1][:2] + [g1[1][2] + 0.25 * g1[1][5]] + g1[1][3:7],                             # 1: full BEV, 3/4 of the height: IoU 0.6
          g1[2][:3] + [g1[2][4], g1[2][3], g1[2][5], g1[2][6] + math.pi / 2],                # 2: rotated by pi / 2 on the same footprint
          g1[3][:6] + [g1[3][6] + math.pi + 0.04],                                          # 3: opposite orientation (the flip)
          [20.05, 10.1, 0.3, 2.0, 4.0, 1.6, 1.12],                                          # 4: label 1, best gt is the class-2 one
          _moved(g1[0], r, 0.45), _moved(g1[1], r, 0.5), _moved(g1[3], r, 0.4)]            # 5-7: hard background
    l1 = [1, 2, 3, 1, 1, 1, 2, 1]
    for k in range(COUNTS[1] - len(c1)):
        c1.append([r.uniform(-30, 30), -30.0 - 6.0 * k, r.uniform(-0.5, 0.5), 2.0, 4.4, 1.6, r.uniform(-math.pi, math.pi)])
        l1.append(1 + k % 3)
    rois[1, :COUNTS[1]], labels[1, :COUNTS[1]] = np.asarray(c1), np.asarray(l1)

    # sample 2: no gt at all
    for k in range(COUNTS[2]):
        rois[2, k] = [r.uniform(-30, 30), r.uniform(-30, 30), r.uniform(-0.5, 0.5), r.uniform(1.8, 2.2), r.uniform(4, 4.8), 1.6, r.uniform(-math.pi, math.pi)]
        labels[2, k] = 1 + k % 3
    scores = np.zeros((B, R))
    for i, n in enumerate(COUNTS):
        scores[i, :n] = r.uniform(0.1, 1.0, n)
    return rois.astype(np.float32), labels, scores.astype(np.float32), gt.astype(np.float32)


def inputs(cs, fgonly=False):
    """-> dict of torch tensors: rois (B', R, cs), roi_labels int64, roi_scores, roi_features (B', R, F), gt (B', N, cs + 1) -- zero rows at
    the end, zero padding slots -- and the draws u_fg (B', R), u_bg (B', M); B' = 1 for the foreground-only case"""
    rois, labels, scores, gt = _inputs7()
    r = np.random.default_rng(777 + cs)
    if cs == 9:      # [x, y, z, w, l, h, rot, vx, vy] and [.., rot, vx, vy, class]
        live = (labels > 0)[..., None]
        rois = np.concatenate([rois, r.uniform(-3, 3, (B, R, 2)).astype(np.float32) * live], 2)
        gl = (gt[..., 7:] > 0)
        gt = np.concatenate([gt[..., :7], r.uniform(-3, 3, (B, N, 2)).astype(np.float32) * gl, gt[..., 7:]], 2)
    feats = r.standard_normal((B, R, F)).astype(np.float32) * (labels > 0)[..., None]
    u_fg, u_bg = r.random((B, R), dtype=np.float32), r.random((B, M), dtype=np.float32)
    if fgonly:
        fg = [k for k in range(COUNTS[0]) if k in FG_SLOTS_0()]
        pick = [fg[k % len(fg)] for k in range(R)]
        rois, labels, scores, feats, gt = rois[0:1, pick], labels[0:1, pick], scores[0:1, pick], feats[0:1, pick], gt[0:1]
        u_fg, u_bg = u_fg[0:1], u_bg[0:1]
    t = torch.from_numpy
    return dict(rois=t(np.ascontiguousarray(rois)), roi_labels=t(np.ascontiguousarray(labels)), roi_scores=t(np.ascontiguousarray(scores)),
                roi_features=t(np.ascontiguousarray(feats.astype(np.float32))), gt=t(np.ascontiguousarray(gt)), u_fg=t(u_fg.copy()), u_bg=t(u_bg.copy()))


_FG0 = None


def FG_SLOTS_0():
    """the ROI slots of sample 0 at IoU >= 0.55 (all-class and by-class agree there: every ROI carries its gt's class)"""
    global _FG0
    if _FG0 is None:
        rois, labels, _, gt = _inputs7()
        mo, _ = max_iou(torch.from_numpy(rois[0:1]), torch.from_numpy(labels[0:1]), torch.from_numpy(gt[0:1]), False)
        _FG0 = [int(k) for k in torch.nonzero(mo[0] >= 0.55).view(-1)]
    return _FG0


# ------------------------------------------------------------------------------------------------ the restatement
def kept_rows(gt_b: torch.Tensor) -> int:
    """the gt list is cut after the last row that is not all zeros; at least one row is kept"""
    nz = torch.nonzero((gt_b != 0).any(1)).view(-1)
    return int(nz[-1]) + 1 if len(nz) else 1


def iou_matrix(rois7: torch.Tensor, gts7: torch.Tensor, exact=False) -> torch.Tensor:
    from oracle.e2e_loss_oracle import iou3d_pairs, iou3d_pairs_exact
    n, m = len(rois7), len(gts7)
    a = rois7.numpy()[:, None, :].repeat(m, 1).reshape(n * m, 7)
    b = gts7.numpy()[None, :, :].repeat(n, 0).reshape(n * m, 7)
    res = (iou3d_pairs_exact if exact else iou3d_pairs)(a, b)
    return torch.from_numpy(np.asarray(res, np.float64 if exact else np.float32).reshape(n, m))


def max_iou(rois, roi_labels, gt, by_class, exact=False):
    """pn_roi_max_iou3d_f32 -> max_overlaps (B, R), gt_assignment (B, R) int32"""
    b, r, _ = rois.shape
    mo, ga = torch.zeros((b, r), dtype=torch.float64 if exact else torch.float32), torch.zeros((b, r), dtype=torch.int32)
    for i in range(b):
        g = gt[i, :kept_rows(gt[i])]
        iou = iou_matrix(rois[i, :, :7], g[:, :7], exact)
        iou = torch.where(torch.isnan(iou), torch.zeros_like(iou), iou)
        if by_class:
            same = g[:, -1].long()[None, :] == roi_labels[i][:, None]
            iou = torch.where(same, iou, torch.full_like(iou, -1.0))
        best, idx = iou.max(1)                   # ties: the lowest index
        idx = (iou == best[:, None]).float().argmax(1)
        found = best >= 0
        mo[i], ga[i] = torch.where(found, best, torch.zeros_like(best)), torch.where(found, idx, torch.zeros_like(idx)).int()
    return mo, ga


def draw_index(u: torch.Tensor, n: int) -> torch.Tensor:
    """min(int(floorf(u * n)), n - 1) with an f32 product"""
    return torch.clamp(torch.floor(u.float() * torch.tensor(float(n), dtype=torch.float32)).long(), 0, n - 1)


def sample_inds(mo_b: torch.Tensor, u_fg_b: torch.Tensor, u_bg_b: torch.Tensor, cfg) -> torch.Tensor:
    """the draws' contract of the header on one sample's max overlaps -> (M,) ROI slots"""
    m = cfg["ROI_PER_IMAGE"]
    f = lambda v: torch.tensor(v, dtype=torch.float32)      # noqa: E731  (the comparisons run on the f32 thresholds)
    fg = torch.nonzero(mo_b >= f(min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"]))).view(-1)
    easy = torch.nonzero(~(mo_b >= f(cfg["CLS_BG_THRESH_LO"]))).view(-1)
    hard = torch.nonzero((mo_b < f(cfg["REG_FG_THRESH"])) & (mo_b >= f(cfg["CLS_BG_THRESH_LO"]))).view(-1)
    if len(fg) and not len(hard) + len(easy):
        return fg[draw_index(u_bg_b[:m], len(fg))]
    k = min(int(np.round(cfg["FG_RATIO"] * m)), len(fg))
    picks = [fg[torch.argsort(u_fg_b[:len(fg)], stable=True)[:k]]]
    need = m - k
    if len(hard) and len(easy):
        hard_num = min(int(need * cfg["HARD_BG_RATIO"]), len(hard))
    else:
        hard_num = need if len(hard) else 0
    if hard_num:
        picks.append(hard[draw_index(u_bg_b[:hard_num], len(hard))])
    if need - hard_num:
        picks.append(easy[draw_index(u_bg_b[hard_num:need], len(easy))])
    return torch.cat(picks)


def py_mod(a: torch.Tensor, b: float) -> torch.Tensor:
    return torch.remainder(a, b)


def targets(inp, cfg, max_overlaps=None, gt_assignment=None, dtype=torch.float32):
    """pn_roi_max_iou3d_f32 + pn_roi_sample_targets_f32 -> the targets dict (float32 / int64 / int32 torch tensors).  ``dtype``: the
    arithmetic of the two computed outputs, gt_of_rois and rcnn_cls_labels (float64: the same restatement on the same float32 inputs,
    thresholds and constants); the selection and the copied rows do not depend on it"""
    rois, labels, scores, feats, gt = inp["rois"], inp["roi_labels"], inp["roi_scores"], inp["roi_features"], inp["gt"]
    b, _, cs = rois.shape
    if max_overlaps is None:
        max_overlaps, gt_assignment = max_iou(rois, labels, gt, cfg["SAMPLE_ROI_BY_EACH_CLASS"])
    inds = torch.stack([sample_inds(max_overlaps[i], inp["u_fg"][i], inp["u_bg"][i], cfg) for i in range(b)])
    take = lambda t: torch.stack([t[i][inds[i]] for i in range(b)])      # noqa: E731
    s_rois, iou = take(rois), take(max_overlaps)
    src = torch.stack([gt[i][gt_assignment[i].long()[inds[i]]] for i in range(b)])
    c32 = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)      # noqa: E731  (a Python double rounded to f32 once)
    two_pi, pi, half_pi, three_half_pi = c32(2 * math.pi), c32(math.pi), c32(math.pi * 0.5), c32(math.pi * 1.5)
    rois_out, src_out, iou_out = s_rois, src, iou
    s_rois, src, iou = s_rois.to(dtype), src.to(dtype), iou.to(dtype)
    ry = s_rois[..., 6] - torch.floor(s_rois[..., 6] / two_pi + 0.5) * two_pi
    enc = src.clone()
    d = src[..., :3] - s_rois[..., :3]
    ca, sa = torch.cos(-ry), torch.sin(-ry)
    enc[..., 0] = d[..., 0] * ca + d[..., 1] * sa
    enc[..., 1] = d[..., 0] * (-sa) + d[..., 1] * ca
    enc[..., 2] = d[..., 2]
    enc[..., 3:6] = src[..., 3:6] - s_rois[..., 3:6]
    if cs == 9:
        enc[..., 7:9] = src[..., 7:9] - s_rois[..., 7:9]
    h = py_mod(src[..., 6] - ry, two_pi)
    flip = (h > half_pi) & (h < three_half_pi)
    h = torch.where(flip, py_mod(h + pi, two_pi), h)
    h = torch.where(h > pi, h - two_pi, h)
    enc[..., 6] = torch.clamp(h, -half_pi, half_pi)
    f = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)      # noqa: E731
    fgt, bgt = f(cfg["CLS_FG_THRESH"]), f(cfg["CLS_BG_THRESH"])
    if cfg["CLS_SCORE_TYPE"] == "roi_iou":
        lab = (iou > fgt).to(dtype)
        mid = ~(iou > fgt) & ~(iou < bgt)
        lab = torch.where(mid, (iou - bgt) / f(cfg["CLS_FG_THRESH"] - cfg["CLS_BG_THRESH"]), lab)
    else:
        lab = (iou > fgt).to(dtype)
        lab = torch.where((iou > bgt) & (iou < fgt), torch.full_like(lab, -1.0), lab)
    return dict(sampled_inds=inds.int(), rois=rois_out, roi_labels=take(labels), roi_scores=take(scores), gt_iou_of_rois=iou_out, roi_features=take(feats),
                gt_of_rois_src=src_out, gt_of_rois=enc, reg_valid_mask=(iou > f(cfg["REG_FG_THRESH"])).long(), rcnn_cls_labels=lab,
                max_overlaps=max_overlaps, gt_assignment=gt_assignment)


TARGET_KEYS = ("sampled_inds", "rois", "roi_labels", "roi_scores", "gt_iou_of_rois", "roi_features", "gt_of_rois_src", "gt_of_rois", "reg_valid_mask",
               "rcnn_cls_labels")


def roi_loss(rcnn_cls, rcnn_reg, cls_labels, gt_of_rois, reg_valid_mask, cw, cls_weight=1.0, reg_weight=1.0):
    """pn_roi_loss_f32's forward in torch (any float dtype; autograd gives the gradients) -> (rcnn_loss, rcnn_loss_cls, rcnn_loss_reg)"""
    dt = rcnn_cls.dtype
    x, y = rcnn_cls.reshape(-1), cls_labels.reshape(-1).to(dt)
    p = torch.sigmoid(x)
    valid = (y >= 0).to(dt)
    bce = -(y * torch.clamp(torch.log(p), min=-100.0) + (1 - y) * torch.clamp(torch.log(1 - p), min=-100.0))
    l_cls = (bce * valid).sum() / torch.clamp(valid.sum(), min=1.0) * cls_weight
    cs = rcnn_reg.shape[-1]
    fg = (reg_valid_mask.reshape(-1) > 0).to(dt)
    l1 = (rcnn_reg - gt_of_rois.reshape(-1, gt_of_rois.shape[-1])[:, :cs].to(dt)).abs() * torch.tensor(list(cw), dtype=dt)
    l_reg = (l1 * fg[:, None]).sum() / torch.clamp(fg.sum(), min=1.0) * reg_weight
    return l_cls + l_reg, l_cls, l_reg
