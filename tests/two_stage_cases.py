"""Seeded inputs and float64 references for tests/test_hip_two_stage_kernels.py (the five second-stage kernels at the sizes of the
reference's two-stage configs) and the conditions on them that tests/test_two_stage_cases_cpu.py asserts without a GPU.

Nothing here restates a kernel a second time: the numbers come from tests/two_stage_ref.py and tests/two_stage_train_ref.py, evaluated
in float32 (as the kernels compute) and in float64 on the same float32 inputs; the selection (``sample_inds``, ``kept_rows``, the max / tie
rule of ``max_iou``) is theirs.  Every case is built once per process and shared (``functools.lru_cache``); the tests do not modify it.

The metric of the numeric comparisons is ``row_err``: per output row max |got - ref64| / max |ref64|, the maximum over the rows; e32 is
that metric of the float32 restatement, and a kernel is allowed FACTOR * e32 (tests/test_hip_setblock_kernels.py).  A row whose float64
reference is exactly zero must be exactly zero.  One kind of row has no scale of its own: an ROI slot ALL of whose sample points lie left
or right of the map, or any point on a map one pixel wide.  There both column indices clamp to the same pixel, the four products cancel
in pairs, the true value is 0 and what float32 or float64 return is the rounding of that cancellation (1e-7 or 1e-16 of the products).
For these rows alone the scale of the metric is the row's max of sum |product| (``sample_map(magnitude=True)``) instead of max |ref64|."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from tests import two_stage_ref as TR2
from tests import two_stage_train_ref as TR

FACTOR = 8.0                   # of tests/test_hip_setblock_kernels.py
F32, F64 = torch.float32, torch.float64
U_MAX = 1 - 2.0 ** -24         # the largest float32 draw below 1


def row_err(got, ref64, scale=None):
    """max over rows of max_c |got - ref64| / max_c |ref64| (or / ``scale``, one value per row); a row of scale 0 must be equal"""
    last = ref64.shape[-1]
    d = (got.to(F64) - ref64).abs().reshape(-1, last).amax(-1)
    s = ref64.abs().reshape(-1, last).amax(-1) if scale is None else scale.reshape(-1).to(F64)
    zero = s == 0
    if bool(d[zero].any()) or not bool(torch.isfinite(d).all()):
        return float("inf")
    return float((d[~zero] / s[~zero]).max()) if bool((~zero).any()) else 0.0


# ------------------------------------------------------------------------------------------------ pn_roi_bev_gather_f32
#               (B, H, W, C, P, cols, cap_in, max_rois): counts
GATHER_CASES = {
    (2, 24, 40, 260, 5, 9, 12, 12): (12, 9),          # 65 channel vectors; five points with the rotation in column 8
    (1, 6, 5, 4, 5, 7, 3, 3): (3,),                   # one vector; 15 items: the last block of four waves is not full
    (3, 24, 40, 64, 1, 7, 501, 503): (508, 0, 250),   # max_rois > cap_in; cap_in + 7 acts as cap_in; item counts no multiple of 4
    (1, 1, 7, 8, 5, 7, 4, 4): (4,),                   # a map one pixel high
    (1, 7, 1, 8, 5, 7, 4, 4): (4,),                   # a map one pixel wide
}
GATHER_NEGATIVE = ((2, 24, 40, 260, 5, 9, 12, 12), (-3, 12))      # a negative count acts as 0
INTEGER_MARGIN = 1e-4


def map_coords(boxes64, num_point):
    """(n, cols) float64 boxes -> the (n, P) map coordinates x, y of their sample points"""
    return TR2.cells_of(TR2.box_points(boxes64, num_point))


def off_integers(boxes, num_point):
    """(n,) bool: no sample point of the box has a float64 map coordinate within INTEGER_MARGIN of an integer (floor agrees in f32 and f64)"""
    x, y = map_coords(torch.as_tensor(np.asarray(boxes, np.float32)).to(F64), num_point)
    far = lambda v: (v - torch.round(v)).abs() > INTEGER_MARGIN      # noqa: E731
    return (far(x) & far(y)).all(1)


@functools.lru_cache(maxsize=None)
def gather_case(shape, counts=None):
    """-> dict: the float32 inputs (rows at or past the effective count NaN / -1), ``counts`` as given to the kernel, ``eff`` the counts
    it must act on, the float64 reference, the float32 one, ``scale`` (see the module's docstring) and e32"""
    b, h, w, c, p, cols, cap, r = shape
    counts = GATHER_CASES[shape] if counts is None else counts
    eff = [min(max(n, 0), cap) for n in counts]
    g = np.random.default_rng(sum(shape) * 31 + len(counts) + (counts[0] < 0))
    x_lo, x_hi = TR2.PC_START[0] - 1.0, TR2.PC_START[0] + w * TR2.VOXEL_SIZE[0] * TR2.OUT_STRIDE + 1.0      # a region wider than the map
    y_lo, y_hi = TR2.PC_START[1] - 1.0, TR2.PC_START[1] + h * TR2.VOXEL_SIZE[1] * TR2.OUT_STRIDE + 1.0
    boxes = np.full((b, cap, cols), np.nan, np.float32)
    scores, labels = np.full((b, cap), np.nan, np.float32), np.full((b, cap), -1, np.int64)
    redrawn = 0

    standard = (h, w) == (24, 40)                                # the map the crafted boxes were made for
    size = min(1.0, w / 40, h / 24)                              # boxes of a smaller map shrink with it: some of their points stay inside

    def seeded():
        return [g.uniform(x_lo, x_hi), g.uniform(y_lo, y_hi), g.uniform(-1, 1), size * g.uniform(0.6, 2.4), size * g.uniform(0.6, 5.0), g.uniform(1, 2),
                g.uniform(-2.5 * math.pi, 2.5 * math.pi)]

    for i, n in enumerate(eff):
        rows = [list(k) for k in TR2.CRAFTED[:n - min(n // 2, 5) if standard else 1]]      # the crafted boxes first, then seeded ones
        while len(rows) < n:
            row = seeded()
            while not bool(off_integers([row], 5)[0]):
                row, redrawn = seeded(), redrawn + 1
            rows.append(row)
        rows = np.asarray(rows, np.float32).reshape(n, 7)
        if cols == 9:                       # the head's order: [x, y, z, w, l, h, vx, vy, rot]
            rows = np.concatenate([rows[:, :6], g.uniform(-3, 3, (n, 2)).astype(np.float32), rows[:, 6:]], 1)
        boxes[i, :n], scores[i, :n], labels[i, :n] = rows, g.uniform(0.1, 1.0, n).astype(np.float32), g.integers(0, 3, n)
    t = torch.from_numpy
    k = dict(shape=shape, boxes=t(boxes), scores=t(scores), labels=t(labels), counts=torch.tensor(counts, dtype=torch.int32), eff=eff,
             bev=t(g.standard_normal((b, h, w, c)).astype(np.float32)), redrawn=redrawn)
    e = torch.tensor(eff, dtype=torch.int32)
    k["ref32"] = TR2.gather(k["boxes"], k["scores"], k["labels"], e, k["bev"], p, cols, r)
    k["ref64"] = TR2.gather(k["boxes"].to(F64), k["scores"], k["labels"], e, k["bev"].to(F64), p, cols, r)
    mag = TR2.gather(k["boxes"].to(F64), k["scores"], k["labels"], e, k["bev"].to(F64), p, cols, r, magnitude=True)[3]
    # the rows that are zero but for rounding: every point's two column indices clamp to the same pixel
    scale = k["ref64"][3].abs().amax(-1)
    for i, n in enumerate(eff):
        if n:
            x, _ = map_coords(k["boxes"][i, :n].to(F64), p)
            fx = torch.floor(x)
            null = ((fx.clamp(0, w - 1) == (fx + 1).clamp(0, w - 1))).all(1)
            scale[i, :n] = torch.where(null, mag[i, :n].amax(-1), scale[i, :n])
    k["scale"] = scale
    k["e32"] = row_err(k["ref32"][3], k["ref64"][3], scale)
    return k


# ------------------------------------------------------------------------------------------------ pn_roi_refine_f32
#              (B, R): counts
REFINE_CASES = {(3, 500): (0, 500, 505), (1, 257): (257,), (2, 1): (-1, 1)}
REFINE_ROTATIONS = (0.4, 2.0, -2.5, -0.7, 7.0, -8.0, 2 * math.pi + 2.5, -2 * math.pi - 1.0)      # four quadrants, and beyond +-2 pi


@functools.lru_cache(maxsize=None)
def refine_case(shape, cs):
    """-> the ROI buffers as pn_roi_bev_gather_f32 leaves them ([x, y, z, w, l, h, rot, vx, vy]) but with NaN / -1 at and past the
    effective count (never read), rcnn_cls (B * R, 1), rcnn_reg (B * R, cs), the two references and e32 of boxes and scores"""
    b, r = shape
    counts = REFINE_CASES[shape]
    eff = [min(max(n, 0), r) for n in counts]
    g = np.random.default_rng(1000 * b + r + cs)
    rois, rs, rl = np.full((b, r, cs), np.nan, np.float32), np.full((b, r), np.nan, np.float32), np.full((b, r), -1, np.int64)
    cls, reg = (g.standard_normal((b, r)) * 2).astype(np.float32), (g.standard_normal((b, r, cs)) * 0.5).astype(np.float32)
    for i, n in enumerate(eff):
        rows = np.concatenate([g.uniform(-40, 40, (n, 2)), g.uniform(-1, 1, (n, 1)), g.uniform(0.6, 5.0, (n, 3)), g.uniform(-3 * math.pi, 3 * math.pi, (n, 1)),
                               g.uniform(-3, 3, (n, cs - 7))], 1)
        m = min(n, len(REFINE_ROTATIONS))
        rows[:m, 6] = REFINE_ROTATIONS[(i % 2) * (len(REFINE_ROTATIONS) - m):][:m]      # a single live row takes another rotation per sample
        rois[i, :n], rs[i, :n], rl[i, :n] = rows, g.uniform(0.1, 1.0, n), g.integers(1, 4, n)
        if n >= 3:
            cls[i, 0], cls[i, 1], rs[i, 2] = 100.0, -100.0, 0.0
    t = torch.from_numpy
    k = dict(shape=shape, cs=cs, rois=t(rois), roi_scores=t(rs), roi_labels=t(rl), counts=torch.tensor(counts, dtype=torch.int32), eff=eff,
             cls=t(cls).reshape(-1, 1), reg=t(reg).reshape(-1, cs))
    e = torch.tensor(eff, dtype=torch.int32)
    k["ref32"] = TR2.refine(k["rois"], k["roi_scores"], k["roi_labels"], e, k["cls"], k["reg"])
    k["ref64"] = TR2.refine(k["rois"].to(F64), k["roi_scores"].to(F64), k["roi_labels"], e, k["cls"].to(F64), k["reg"].to(F64))
    k["e32_boxes"] = row_err(k["ref32"][0], k["ref64"][0])
    k["e32_scores"] = row_err(k["ref32"][1], k["ref64"][1])      # a row: one sample's scores
    return k


# ------------------------------------------------------------------------------------------------ gts and ROIs for the training kernels
def grid_gts(g, n, first_classes=(1, 2, 3)):
    """n gt rows [x, y, z, w, l, h, rot, class] on a 13-wide grid of 6 m x 7 m cells: no two of them touch (the diagonal is below 5.3 m)"""
    rows = []
    for k in range(n):
        rows.append([-36.0 + 6.0 * (k % 13) + g.uniform(-0.3, 0.3), -31.5 + 7.0 * (k // 13) + g.uniform(-0.3, 0.3), g.uniform(-0.5, 0.5), g.uniform(1.8, 2.2),
                     g.uniform(4.0, 4.8), g.uniform(1.5, 1.8), g.uniform(-math.pi, math.pi), first_classes[k % 3]])
    return np.asarray(rows)


FG_SHIFT, HARD_SHIFT, EASY_SHIFT = (0.03, 0.2), (0.3, 0.6), (0.75, 0.9)


def roi_of_kind(g, gts, kind, k):
    """one ROI [x, y, z, w, l, h, rot] and its label: 'fg' / 'hard' / 'near' (a small non-zero overlap) next to gt k, 'far' away from all"""
    if kind == "far":
        return [80.0 + g.uniform(0, 40), g.uniform(-40, 40), g.uniform(-0.5, 0.5), 2.0, 4.4, 1.6, g.uniform(-math.pi, math.pi)], 1 + k % 3
    lo, hi = dict(fg=FG_SHIFT, hard=HARD_SHIFT, near=EASY_SHIFT)[kind]
    gt = gts[k]
    return TR._moved(list(gt[:7]), g, g.uniform(lo, hi), drot=g.uniform(-0.03, 0.03)), int(gt[7])


def with_velocity(g, rois, gt, cs):
    """7-column ROIs and 8-column gts -> code_size ``cs``: [.., rot, vx, vy] and [.., rot, vx, vy, class]; zero rows stay zero"""
    if cs == 7:
        return rois, gt
    live_r, live_g = (rois != 0).any(-1, keepdims=True), (gt != 0).any(-1, keepdims=True)
    rois = np.concatenate([rois, g.uniform(-3, 3, rois.shape[:-1] + (2,)).astype(np.float32) * live_r], -1)
    gt = np.concatenate([gt[..., :7], g.uniform(-3, 3, gt.shape[:-1] + (2,)).astype(np.float32) * live_g, gt[..., 7:]], -1)
    return rois.astype(np.float32), gt.astype(np.float32)


def iou32(rois7, gts7):
    return TR.iou_matrix(torch.as_tensor(rois7)[:, :7].contiguous(), torch.as_tensor(gts7)[:, :7].contiguous())


# ------------------------------------------------------------------------------------------------ pn_roi_max_iou3d_f32
IOU_CASES = ((2, 501, 130), (1, 3, 65))
IOU_GAP = 1e-3                 # between the best and the second-best competing IoU of an ROI (unless the two gt rows are bit-identical)
BEST_ROWS = (0, 63, 64, 65, 127, 128)
TWINS = ((10, 74), (20, 45))   # bit-identical gt rows: the same lane of two passes, and two lanes
ZERO_ROW = 70                  # an all-zero gt row with non-zero rows behind it
REDRAW_CAP = 0.01


def shifted(rois, sign):
    """the ROIs with x moved by 1e-6 (by one float32 step where 1e-6 is less than that)"""
    out = rois.copy()
    x = rois[:, 0]
    moved = (x.astype(np.float64) + sign * 1e-6).astype(np.float32)
    out[:, 0] = np.where(moved == x, np.nextafter(x, np.float32(sign * np.inf)), moved)
    return out


def competing_gap(iou, roi_labels, gt_b, by_class):
    """per ROI: best minus second-best competing IoU; infinite where there is no runner-up but bit-identical rows, and where the best
    is exactly 0 (no overlap at all is exact in any arithmetic: the lowest competing index is the answer)"""
    n = iou.shape[1]
    v = torch.nan_to_num(iou.clone().double(), nan=0.0)
    if by_class:
        v[gt_b[:n, -1].long()[None, :] != roi_labels[:, None]] = -1.0
    best, idx = v.max(1)
    same = (gt_b[:n, None, :] == gt_b[None, :n, :]).all(-1)      # (n, n): bit-identical rows (no NaN, no -0 among the gts)
    rest = torch.where(same[idx] | (v < 0), torch.full_like(v, -float("inf")), v)
    gap = best - rest.amax(1)
    gap[best <= 0] = float("inf")
    return gap


@functools.lru_cache(maxsize=None)
def iou_geometry(shape):
    """the 7-column content of a max-IoU case -> rois (B, R, 7), labels (B, R), gt (B, N, 8), ``slots``: what some ROI slots of sample 0 are
    for, the per-sample f32 IoU matrices, and the number of ROIs the generator replaced (discontinuity of the containment margin, or a
    runner-up within IOU_GAP)"""
    b, r, n = shape
    g = np.random.default_rng(4242 + r)
    gt = np.zeros((b, n, 8), np.float32)
    rois, labels = np.zeros((b, r, 7), np.float32), np.zeros((b, r), np.int64)
    big = n >= 129
    nz = n - 1 if big else n                                    # the last row of the large case is zero: the cut is after row 128
    gt[0, :nz] = grid_gts(g, nz).astype(np.float32)
    slots = {}
    if big:
        for lo, hi in TWINS:
            gt[0, hi] = gt[0, lo]
        gt[0, ZERO_ROW] = 0
        live = r - 10                                           # ten padding slots of zeros
        plan = [("best", k) for k in BEST_ROWS] + [("twin", lo) for lo, _ in TWINS] + [("twin_hi", hi) for _, hi in TWINS] + [("noclass", 5), ("noclass", 100)]
        plan += [("far", k) for k in range(24)]
    else:
        live = r
        plan = [("best", 64), ("best", 0), ("far", 1)]
    rows_ok = [k for k in range(nz) if not (big and k == ZERO_ROW)]
    while len(plan) < live:
        plan.append((("fg", "hard", "near")[len(plan) % 3], rows_ok[int(g.integers(len(rows_ok)))]))
    replaced = 0

    def draw(what, k):
        kind = dict(best="fg", twin="fg", twin_hi="hard", noclass="fg").get(what, what)
        row, lab = roi_of_kind(g, gt[0], kind, k)
        return np.asarray(row, np.float32), (4 if what == "noclass" else lab)

    for s, (what, k) in enumerate(plan):
        rois[0, s], labels[0, s] = draw(what, k)
        slots.setdefault(what, []).append((s, k))
    if b > 1:                                                   # sample 1: no gt at all
        for s in range(r - 5):
            rois[1, s], labels[1, s] = draw("far" if s % 2 else "fg", s % nz)
    gt_t = torch.from_numpy(gt)
    for _ in range(20):                                         # redraw what sits on a discontinuity or has a close runner-up
        m = iou32(rois[0], gt[0, :nz])
        lt = torch.from_numpy(labels[0])
        bad = (competing_gap(m, lt, gt_t[0], True) < IOU_GAP) | (competing_gap(m, lt, gt_t[0], False) < IOU_GAP)
        for sign in (-1, 1):
            bad |= ((iou32(shifted(rois[0], sign), gt[0, :nz]) - m).abs() > TR.REL).any(1)
        bad = [int(s) for s in torch.nonzero(bad).view(-1) if s < live]
        if not bad:
            break
        for s in bad:
            rois[0, s], labels[0, s] = draw(*plan[s])
            replaced += 1
    return dict(rois=rois, labels=labels, gt=gt, slots=slots, replaced=replaced, live=live, kept=nz)


@functools.lru_cache(maxsize=None)
def iou_case(shape, by_class, cs):
    """-> rois (B, R, cs), roi_labels, gt (B, N, cs + 1) and the restatement's (max_overlaps, gt_assignment) on them"""
    geo = iou_geometry(shape)
    rois, gt = with_velocity(np.random.default_rng(cs), geo["rois"], geo["gt"], cs)
    if shape[2] >= 129:
        for lo, hi in TWINS:
            gt[0, hi] = gt[0, lo]                               # bit-identical with their velocities
    k = dict(rois=torch.from_numpy(rois), roi_labels=torch.from_numpy(geo["labels"]), gt=torch.from_numpy(gt), geo=geo)
    k["max_overlaps"], k["gt_assignment"] = TR.max_iou(k["rois"], k["roi_labels"], k["gt"], by_class)
    return k


# ------------------------------------------------------------------------------------------------ pn_roi_sample_targets_f32
def spread(total, count, offset=0):
    """``count`` slots spread evenly over range(total)"""
    return sorted({(offset + (i * total) // count) % total for i in range(count)}) if count else []


def kinds_of(r, nf, nh, fg_slots=None):
    """a list of R kinds: nf 'fg' spread over all the slots (or at ``fg_slots``), nh 'hard' spread over the rest, 'far' / 'near' easy elsewhere"""
    kinds = [None] * r
    for s in (spread(r, nf) if fg_slots is None else fg_slots):
        kinds[s] = "fg"
    rest = [s for s in range(r) if kinds[s] is None]
    for i in spread(len(rest), nh, 1):
        kinds[rest[i]] = "hard"
    for n, s in enumerate(s for s in range(r) if kinds[s] is None):
        kinds[s] = "near" if n % 4 == 0 else "far"
    return kinds


# name: (B, R, N, M, F), score type, code size, per sample (nf, n_hard) -- the rest is easy background -- and what the case is for
SAMPLER_CASES = {
    "production": ((2, 500, 130, 128, 260), "roi_iou", 7, ((100, 30), (20, 150))),   # 65 feature vectors; n_hard below / above int(need * 0.8)
    "production_cls9": ((2, 500, 130, 128, 260), "cls", 9, ((100, 30), (20, 150))),
    "second_round": ((1, 257, 12, 300, 100), "roi_iou", 9, ((40, 100),)),             # slot 256 is foreground: the carry of one round; M > 256
    "limits": ((1, 2048, 12, 2048, 4), "cls", 7, ((600, 700),)),                      # kMaxRois: 40 KB of LDS
    "rank_strides": ((1, 600, 12, 128, 100), "roi_iou", 7, ((320, 100),)),            # nf > 300: the rank loop takes two strides
    "all_foreground": ((1, 600, 12, 300, 100), "cls", 7, ((600, 0),)),                # every row a draw with replacement, past 256 picks
    "quota_2.5": ((1, 300, 12, 5, 100), "roi_iou", 7, ((30, 40),)),                   # round(2.5) = 2
    "quota_1.5": ((1, 300, 12, 3, 100), "roi_iou", 9, ((30, 40),)),                   # round(1.5) = 2
    "one_row": ((1, 24, 12, 1, 100), "cls", 7, ((5, 6),)),                            # M = 1: the quota is round(0.5) = 0
    "no_foreground": ((1, 300, 12, 128, 100), "roi_iou", 7, ((0, 60),)),
    "hard_only": ((1, 300, 12, 128, 100), "cls", 9, ((0, 300),)),
    "fg_and_hard": ((1, 300, 12, 128, 100), "roi_iou", 7, ((90, 210),)),
    "fg_and_easy": ((1, 300, 12, 128, 100), "roi_iou", 7, ((90, 0),)),
}
FG_SLOTS = {"second_round": spread(256, 39) + [256]}


def sampler_cfg(name):
    shape, score_type = SAMPLER_CASES[name][:2]
    return dict(TR.target_cfg(True, score_type), ROI_PER_IMAGE=shape[3])


def lists_of(mo_b, cfg=TR.TARGET_CFG):
    """(nf, n_hard, n_easy) of one sample's max overlaps, by the sampler's own comparisons"""
    f = lambda v: torch.tensor(v, dtype=F32)      # noqa: E731
    fg = mo_b >= f(min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"]))
    hard = (mo_b < f(cfg["REG_FG_THRESH"])) & (mo_b >= f(cfg["CLS_BG_THRESH_LO"]))
    return int(fg.sum()), int(hard.sum()), int((~(mo_b >= f(cfg["CLS_BG_THRESH_LO"]))).sum())


def off_thresholds(mo):
    return torch.stack([(mo - t).abs() > TR.MARGIN for t in TR.THRESHOLDS]).all(0)


@functools.lru_cache(maxsize=None)
def sampler_case(name):
    """-> the inputs dict of TR.targets (+ max_overlaps, gt_assignment of the restatement), cfg, the two references, e32 per computed
    output, the kinds asked for and the number of redraws"""
    (b, r, n, m, f), score_type, cs, sizes = SAMPLER_CASES[name]
    g = np.random.default_rng(sum(ord(ch) for ch in name) * 7 + r)
    gt = np.zeros((b, n, 8), np.float32)
    rois, labels = np.zeros((b, r, 7), np.float32), np.zeros((b, r), np.int64)
    kinds, redrawn = [], 0
    for i, (nf, nh) in enumerate(sizes):
        ngt = n - 2                                              # two zero rows at the end
        gt[i, :ngt] = grid_gts(g, ngt).astype(np.float32)
        kinds.append(kinds_of(r, nf, nh, FG_SLOTS.get(name)))
        todo = list(range(r))
        for _ in range(40):
            for s in todo:
                row, labels[i, s] = roi_of_kind(g, gt[i], kinds[i][s], int(g.integers(ngt)))
                rois[i, s] = np.asarray(row, np.float32)
            mo, _ = TR.max_iou(torch.from_numpy(rois[i:i + 1, todo]), torch.from_numpy(labels[i:i + 1, todo]), torch.from_numpy(gt[i:i + 1]), True)
            ok = off_thresholds(mo[0])
            for j, s in enumerate(todo):
                v, kd = float(mo[0, j]), kinds[i][s]
                ok[j] &= (v >= 0.55) if kd == "fg" else (0.1 <= v < 0.55) if kd == "hard" else (v < 0.1)
            todo = [s for j, s in enumerate(todo) if not ok[j]]
            if not todo:
                break
            redrawn += len(todo)
        assert not todo, (name, i, len(todo))
    rois, gt = with_velocity(g, rois, gt, cs)
    u_fg, u_bg = g.random((b, r), dtype=np.float32), g.random((b, m), dtype=np.float32)
    u_fg[:, 1], u_fg[:, 3] = 2.0 ** -10, 2.0 ** -10              # duplicated keys near the front of the order: list position 1 before 3
    if r > 260:
        u_fg[:, 2], u_fg[:, 260] = 2.0 ** -9, 2.0 ** -9           # ... and a pair in two strides of the rank loop
    u_bg[:, 0] = 0.0
    if m >= 4:
        u_bg[:, 1], u_bg[:, m - 2], u_bg[:, m - 1] = U_MAX, 0.0, U_MAX
    t = torch.from_numpy
    inp = dict(rois=t(rois), roi_labels=t(labels), roi_scores=t(g.uniform(0.1, 1.0, (b, r)).astype(np.float32)),
               roi_features=t(g.standard_normal((b, r, f)).astype(np.float32)), gt=t(gt), u_fg=t(u_fg), u_bg=t(u_bg))
    cfg = sampler_cfg(name)
    mo, ga = TR.max_iou(inp["rois"], inp["roi_labels"], inp["gt"], True)
    k = dict(name=name, inp=inp, cfg=cfg, cs=cs, max_overlaps=mo, gt_assignment=ga, kinds=kinds, redrawn=redrawn, sizes=sizes)
    k["ref32"], k["ref64"] = TR.targets(inp, cfg, mo, ga), TR.targets(inp, cfg, mo, ga, dtype=F64)
    k["e32"] = {key: row_err(k["ref32"][key], k["ref64"][key]) for key in ("gt_of_rois", "rcnn_cls_labels")}
    return k


# ------------------------------------------------------------------------------------------------ pn_roi_loss_f32
#            (n, cs, mask pattern, (row stride, cls_col, reg_col))
LOSS_CASES = [(n, cs, "mixed", (12 if cs == 7 else 16, 0, 4)) for n in (1, 255, 256, 257, 512, 1000) for cs in (7, 9)] + [
    (512, 7, "all", (12, 0, 4)), (512, 9, "none", (16, 0, 4)), (512, 7, "beyond256", (12, 0, 4)), (512, 9, "below256", (16, 0, 4)),
    (1000, 9, "mixed", (16, 12, 0)),                          # the classification column behind the regression columns
]


@functools.lru_cache(maxsize=None)
def loss_case(case):
    """-> rcnn_cls (n, 1), rcnn_reg (n, cs), labels (n,) mixing 0, 1, fractions and -1, targets (n, cs + 1), mask (n,) int64, the float64
    reference (three losses, d_cls, d_reg) by autograd and e32 of the gradient rows [d_cls | d_reg]"""
    n, cs, pattern, _ = case
    g = np.random.default_rng(n * 10 + cs + len(pattern))
    cls, reg = (g.standard_normal((n, 1)) * 2).astype(np.float32), (g.standard_normal((n, cs)) * 0.5).astype(np.float32)
    enc = np.concatenate([g.standard_normal((n, cs)) * 0.5, g.integers(1, 4, (n, 1))], 1).astype(np.float32)
    # the fractions keep 0.3 away from sigmoid(logit): p - y is no difference of near-equal numbers (that would put e32 above REL / FACTOR)
    frac = np.mod(1 / (1 + np.exp(-cls[:, 0].astype(np.float64))) + 0.3 + 0.4 * g.random(n), 1.0)
    labels = np.choose(np.arange(n) % 4, [np.zeros(n), np.ones(n), frac, -np.ones(n)]).astype(np.float32)
    rows = np.arange(n)
    mask = dict(mixed=rows % 3 != 1, all=rows >= 0, none=rows < 0, beyond256=rows >= 256, below256=rows < 256)[pattern].astype(np.int64)
    if pattern in ("beyond256", "below256"):                  # the valid classification rows lie on the same side
        labels = np.where(mask > 0, np.abs(labels), -1.0).astype(np.float32)
    t = torch.from_numpy
    k = dict(case=case, cls=t(cls), reg=t(reg), labels=t(labels), enc=t(enc), mask=t(mask))
    w = TR.LOSS_CFG["LOSS_WEIGHTS"]

    def run(dt):
        c, r_ = k["cls"].to(dt).requires_grad_(), k["reg"].to(dt).requires_grad_()
        loss = TR.roi_loss(c, r_, k["labels"], k["enc"], k["mask"], TR.code_weights(cs), w["rcnn_cls_weight"], w["rcnn_reg_weight"])
        loss[0].backward()
        return [float(v.detach()) for v in loss], torch.cat([c.grad, r_.grad], 1)

    k["loss64"], k["d64"] = run(F64)
    k["loss32"], d32 = run(F32)
    k["e32"] = row_err(d32, k["d64"])
    return k


# ------------------------------------------------------------------------------------------------ e32 of the small cases
SMALL = 64


def pooled(own, population):
    """e32 of a case with fewer than SMALL output rows: the error of a row is led by one or two rounded numbers, so the float32
    restatement's error on a handful of rows is a few draws that can lie ten times below the typical one (1e-9 on the single live row of
    refine (2, 1)).  As tests/test_hip_setblock_kernels.py does for LayerNorm on 1 and 3 rows, such a case takes the maximum of its own
    e32 and that of the kernel's largest case of the same code size: the same arithmetic on a population of the same distribution"""
    return max(own, population)


def refine_e32(shape, cs):
    k, pop = refine_case(shape, cs), refine_case((3, 500), cs)
    if shape[0] * shape[1] >= SMALL:
        return k["e32_boxes"], k["e32_scores"]
    return pooled(k["e32_boxes"], pop["e32_boxes"]), pooled(k["e32_scores"], pop["e32_scores"])


def sampler_e32(name):
    k = sampler_case(name)
    if SAMPLER_CASES[name][0][3] >= SMALL:
        return k["e32"]
    pop = sampler_case("production" if k["cs"] == 7 else "production_cls9")
    return {key: pooled(v, pop["e32"][key]) for key, v in k["e32"].items()}


def loss_e32(case):
    k = loss_case(case)
    return k["e32"] if case[0] >= SMALL else pooled(k["e32"], loss_case((1000, case[1], "mixed", (12 if case[1] == 7 else 16, 0, 4)))["e32"])
