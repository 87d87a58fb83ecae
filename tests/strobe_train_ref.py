"""Host restatement (numpy) of STROBE's training targets, written from the description of `pn_assign_heatmap_cart_sectors_f32` in
include/partner_hip.h, and the seeded box sets the golden (tests/golden/make_golden_strobe_train.py) and the tests share.  The golden
comes from the reference's own ``voxelize_streaming_cart`` + ``AssignLabel.assign_centerpoint``; this restatement is held to it by
tests/test_strobe_train_cpu.py and serves the device tests for the box counts that are not in the golden.

  sector_targets     one sample's boxes -> per sector (hm, ind, mask, cat, anno_box)
  stacked_targets    a batch -> the five arrays of the nsectors * B stacked samples, sector-major
  group_by_class     the stable class grouping of assign_centerpoint (the order the device entry's caller passes)
"""
from __future__ import annotations

import numpy as np

try:
    from tests.strobe_ref import CART_RANGE, CART_VOXEL, sector_grid
except ImportError:      # run from tests/golden with tests/ on the path
    from strobe_ref import CART_RANGE, CART_VOXEL, sector_grid

F32 = np.float32
CLASSES, OVERLAP, MIN_RADIUS = 10, 0.1, 2
# seeded sets of one sample each per seed: "mixed" has an empty sample, "dense" keeps more than max_objs boxes in some sectors, "train" is the
# set the golden's training iteration takes (4 sectors)
TARGET_SETS = {"mixed": dict(seeds=(5142, 5103), counts=(23, 0), max_objs=32), "dense": dict(seeds=(5111, 5112), counts=(90, 41), max_objs=12),
               "train": dict(seeds=(5121, 5122), counts=(14, 9), max_objs=32)}


def osf_of(nsectors: int) -> int:
    """the out_size_factor of the target tests on the 64 x 64 grid: the map is 8 x 8 (one sector), 8 x 4 (two) and, at the reduced model's
    factor 4, 8 x 8 (four)"""
    return 4 if nsectors == 4 else 8


def set_samples(name: str):
    """-> the samples [(boxes, classes)] of a seeded set, grouped by class"""
    t = TARGET_SETS[name]
    return [group_by_class(*random_boxes(n, seed)) for seed, n in zip(t["seeds"], t["counts"])]


def random_boxes(n: int, seed: int, r_max: float = 70.0):
    """(n, 9) float32 [x, y, z, l, w, h, vx, vy, yaw] and (n,) int32 classes 1..CLASSES; some centres lie outside the grid's circle"""
    r = np.random.default_rng(seed)
    rho, phi = r.uniform(0.5, r_max, n), r.uniform(-np.pi, np.pi, n)
    boxes = np.stack([rho * np.cos(phi), rho * np.sin(phi), r.uniform(-3, 1, n), r.uniform(0.4, 12.0, n), r.uniform(0.4, 6.0, n), r.uniform(0.5, 4.0, n),
                      r.uniform(-8, 8, n), r.uniform(-8, 8, n), r.uniform(-7.0, 7.0, n)], 1).astype(F32)
    return boxes.reshape(n, 9), r.integers(1, CLASSES + 1, n).astype(np.int32)


def exact_boxes():
    """centres whose rotation involves only zeros: azimuth exactly 0 (rows 0 and 3: kept by BOTH sectors that meet there -- and, with two or
    four sectors, on the outer edge of either map, so they take a slot and are not drawn), y = +0.0 with x < 0 (float32 azimuth +pi, above
    the float64 pi: kept by no sector) and y = -0.0 with x < 0 (below -pi: kept by none).  The last three rows lie well inside a sector
    (third, fourth and second quadrant of four; rotations by multiples of pi / 2): with two and four sectors the ones next to azimuth 0 take
    their slot behind rows 0 and 3, which shows that both ends of the azimuth range are inclusive"""
    boxes = np.array([[20.0, 0.0, -1.0, 4.0, 2.0, 1.5, 3.0, 0.0, 0.25],
                      [-12.0, 0.0, 0.5, 5.0, 2.5, 2.0, 0.0, -2.0, 1.0],
                      [-30.0, -0.0, -0.5, 3.0, 1.5, 1.0, 1.0, 0.0, -2.0],
                      [8.0, 0.0, 0.0, 9.0, 3.0, 3.0, 0.0, 0.0, 3.5],
                      [-20.3, -13.7, 0.2, 4.5, 2.0, 1.6, -1.5, 0.5, 0.7],
                      [15.1, 9.3, -0.8, 6.0, 2.4, 2.2, 2.0, 1.0, -1.2],
                      [11.2, -17.4, 0.1, 3.6, 1.8, 1.4, 0.5, -2.5, 2.9]], F32)
    return boxes, np.array([1, 9, 4, 2, 3, 7, 5], np.int32)


def group_by_class(boxes, classes):
    """assign_centerpoint's grouping for a single task (preprocess.py:360-394): the boxes of class 1, then of class 2, ... each in order"""
    order = np.argsort(classes, kind="stable")
    return boxes[order], classes[order]


def gaussian_radius(height, width, mo):
    """center_utils.py:18-38 on float32 scalars (numpy keeps them float32 next to Python numbers)"""
    height, width = F32(height), F32(width)
    b1 = height + width
    c1 = width * height * (1 - mo) / (1 + mo)
    r1 = (b1 + np.sqrt(b1 ** 2 - 4 * c1)) / 2
    b2 = 2 * (height + width)
    c2 = (1 - mo) * width * height
    r2 = (b2 + np.sqrt(b2 ** 2 - 4 * 4 * c2)) / 2
    a3 = 4 * mo
    b3 = -2 * mo * (height + width)
    c3 = (mo - 1) * width * height
    r3 = (b3 + np.sqrt(b3 ** 2 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def draw_gaussian(hm, x, y, radius):
    """center_utils.py:40-64: element-wise maximum with the clipped (2 r + 1)^2 window, sigma = (2 r + 1) / 6"""
    height, width = hm.shape
    sigma = (2 * radius + 1) / 6
    left, right, top, bottom = min(x, radius), min(width - x, radius + 1), min(y, radius), min(height - y, radius + 1)
    if right + left <= 0 or bottom + top <= 0:
        return
    dy, dx = np.ogrid[-top:bottom, -left:right]
    g = np.exp(-(dx * dx + dy * dy) / (2 * sigma * sigma))
    np.maximum(hm[y - top:y + bottom, x - left:x + right], g, out=hm[y - top:y + bottom, x - left:x + right])


def sector_bounds(s: int, nsectors: int):
    """(lo, hi, angle) in float64, one rounding per operation (voxelization.py:192, 230-231, 245)"""
    interval = 2 * np.pi / nsectors
    lo, hi = -np.pi + s * interval, -np.pi + (s + 1) * interval
    return lo, hi, lo + np.pi


def sector_keep(boxes, s, nsectors, pc_range=CART_RANGE):
    """utils.py:19-24: float32 rho and azimuth against the float64 bounds, both azimuth ends inclusive"""
    rg = np.asarray(pc_range, F32)
    r_max = np.float64(np.sqrt(rg[0] * rg[0] + rg[1] * rg[1]))
    lo, hi, _ = sector_bounds(s, nsectors)
    x, y = boxes[:, 0], boxes[:, 1]
    rho = np.sqrt(x * x + y * y).astype(np.float64)
    az = np.arctan2(y, x).astype(np.float64)
    return (rho >= 0) & (rho <= r_max) & (az >= lo) & (az <= hi)


def rotate_boxes(boxes, angle):
    """voxelization.py:245-256 and preprocess.py:399-401 -> (x', y', vx', vy', yaw') ; centre with float32 cos / sin, the velocity in
    float64 (the reference stacks it with a float64 zero column), the yaw: float64 sum rounded to float32, then wrapped in float32"""
    c64, s64 = np.cos(angle), np.sin(angle)
    c, s = F32(c64), F32(s64)
    x, y = boxes[:, 0], boxes[:, 1]
    xr, yr = x * c + y * s, x * (-s) + y * c
    vx, vy = boxes[:, 6].astype(np.float64), boxes[:, 7].astype(np.float64)
    vxr, vyr = (vx * c64 + vy * s64).astype(F32), (vx * (-s64) + vy * c64).astype(F32)
    yaw = (boxes[:, -1].astype(np.float64) + angle).astype(F32)
    period = F32(2 * np.pi)
    yaw = yaw - np.floor(yaw / period + F32(0.5)) * period
    return xr, yr, vxr, vyr, yaw


def sector_targets(boxes, classes, nsectors, max_objs, classes_n=CLASSES, pc_range=CART_RANGE, voxel_size=CART_VOXEL, osf=None, overlap=OVERLAP,
                   min_radius=MIN_RADIUS, details=None):
    """one sample's boxes (grouped by class) -> a list over the sectors of (hm, ind, mask, cat, anno_box).  ``details``: a list that
    receives, per drawn box, (sector, the float32 centre in feature cells (2,), the float32 azimuth)"""
    rg, vs = np.asarray(pc_range, F32), np.asarray(voxel_size, F32)
    grid = sector_grid(np.round((rg[3:] - rg[:3]) / vs).astype(np.int64), nsectors)
    osf = osf_of(nsectors) if osf is None else int(osf)
    fx, fy = grid[0] // osf, grid[1] // osf
    boxes = np.asarray(boxes, F32)
    out = []
    for s in range(nsectors):
        hm = np.zeros((classes_n, fy, fx), F32)
        ind, mask, cat, anno = np.zeros(max_objs, np.int64), np.zeros(max_objs, np.uint8), np.zeros(max_objs, np.int64), np.zeros((max_objs, 10), F32)
        if len(boxes):
            keep = sector_keep(boxes, s, nsectors, pc_range)
            bx, cl = boxes[keep][:max_objs], np.asarray(classes)[keep][:max_objs]
            xr, yr, vxr, vyr, yaw = rotate_boxes(bx, sector_bounds(s, nsectors)[2])
            for k in range(len(bx)):
                w, l = bx[k, 3] / vs[0] / F32(osf), bx[k, 4] / vs[1] / F32(osf)
                if not (w > 0 and l > 0):
                    continue
                radius = max(min_radius, int(gaussian_radius(l, w, overlap)))
                ct = np.array([(xr[k] - rg[0]) / vs[0] / F32(osf), (yr[k] - rg[1]) / vs[1] / F32(osf)], F32)
                ix, iy = int(ct[0]), int(ct[1])      # toward zero
                if not (0 <= ix < fx and 0 <= iy < fy):
                    continue
                draw_gaussian(hm[int(cl[k]) - 1], ix, iy, radius)
                cat[k], ind[k], mask[k] = int(cl[k]) - 1, iy * fx + ix, 1
                anno[k] = [ct[0] - F32(ix), ct[1] - F32(iy), bx[k, 2], np.log(bx[k, 3]), np.log(bx[k, 4]), np.log(bx[k, 5]), vxr[k], vyr[k],
                           np.sin(yaw[k]), np.cos(yaw[k])]
                if details is not None:
                    details.append((s, ct.copy(), np.arctan2(bx[k, 1], bx[k, 0])))
        out.append((hm, ind, mask, cat, anno))
    return out


def stacked_targets(samples, nsectors, max_objs, **kw):
    """samples: a list of (boxes, classes) per sample -> (hm, ind, mask, cat, anno_box) of the nsectors * B stacked samples, sector-major"""
    per = [sector_targets(b, c, nsectors, max_objs, **kw) for b, c in samples]
    return tuple(np.stack([per[b][s][f] for s in range(nsectors) for b in range(len(samples))]) for f in range(5))


def padded_batch(samples, cols=9):
    """samples -> (gt_boxes (B, max_gt, cols) f32, gt_classes (B, max_gt) int32, num_gt (B,) int32): what the device entry takes"""
    max_gt = max(1, max(len(b) for b, _ in samples))
    gb, gc = np.zeros((len(samples), max_gt, cols), F32), np.zeros((len(samples), max_gt), np.int32)
    for i, (b, c) in enumerate(samples):
        gb[i, :len(b)], gc[i, :len(b)] = b, c
    return gb, gc, np.array([len(b) for b, _ in samples], np.int32)
