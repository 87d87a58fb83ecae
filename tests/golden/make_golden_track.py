#!/usr/bin/env python3
"""Golden vectors of the center-based trackers: runs the REFERENCE's two trackers themselves -- ``PubTracker.step_centertrack`` of
tools/nusc_tracking/pub_tracker.py (with track_utils.greedy_assignment) and of tools/waymo_tracking/tracker.py, found through
ref_import.py -- on seeded synthetic sequences and stores the inputs and the reference's ``self.tracks`` after every frame in ``track.npz``.

Container-only: ``python tests/golden/make_golden_track.py``.  Data only.
  per style (``nusc``: 10 detection classes, 7 tracked, score_thresh -inf; ``waymo``: 3 classes, score_thresh 0.75; both max_age 3):
    ``{style}_class_names``, ``{style}_tracking_names`` (str), ``{style}_track_class`` int32 and ``{style}_max_dist`` f32 per detection label
    (from the reference's NUSCENE_CLS_VELOCITY_ERROR / the defaults of waymo_tracking/test.py:34-38), ``{style}_max_age``, ``{style}_score_thresh``
  per sequence ``{tag}`` in nusc_a, nusc_b, waymo_a, waymo_b (8 frames, <= 48 rows, the two of a style with different counts):
    inputs    ``_boxes`` (F, 48, 9) f32 device-list rows (x, y, z, w, l, h, vx, vy, rot), ``_scores``, ``_labels`` int64, ``_count`` int32,
              ``_time_lag`` f64, ``_first`` int32 (1 = the driver resets the tracker before this frame), ``_pose`` (F, 3, 4) f64 lidar -> global
              (waymo_b only: an ego a few km from the origin that drives and turns; the others are global already)
    expected  the table after the frame, padded to the longest: ``_t_ct``, ``_t_tracking`` (F, Tm, 2) f64, ``_t_label``, ``_t_tracking_id``,
              ``_t_age``, ``_t_active``, ``_t_box_id`` (F, Tm) int32, ``_t_count`` (F,), ``_id_count`` (F,).  box_id is -1 where active == 0:
              the reference's coasting dicts keep the row number of the frame they were last seen in, which nothing reads.
  nusc_b has an empty frame and a reset in the middle; waymo_a has detections below score_thresh, matched and unmatched.
The dicts handed to the reference are built as waymo_tracking/test.py builds them: translation and velocity in f64 from the f32 boxes
(pose applied in f64), detection_name, score, box_id.

Decision margins (asserted in f64 against the reference's state BEFORE each step; an object that violates one gets new noise): every
same-class pair keeps |dist - max_dist| >= margin, and every row's best and second-best valid candidates differ by >= margin, with
margin = 1e-3 m, or 8 x the f32 spacing at the largest coordinate for the sequence with a real pose.  With them an f32 or last-bit f64
difference in the arithmetic cannot change a decision, so the tests compare exactly.
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402

CAP, FRAMES = 48, 8
NUSC_CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
WAYMO_CLASSES = ["VEHICLE", "PEDESTRIAN", "CYCLIST"]
WAYMO_MAX_DIST = {"VEHICLE": 0.8, "PEDESTRIAN": 0.4, "CYCLIST": 0.6}


def reference_trackers():
    assert ref_import.reference_available()
    mods = []
    for folder, name in (("nusc_tracking", "pub_tracker"), ("waymo_tracking", "tracker")):
        path = os.path.join(ref_import.REFERENCE_ROOT, "tools", folder)
        sys.path.insert(0, path)            # pub_tracker imports track_utils from its own folder
        mods.append(importlib.import_module(name))
        sys.path.remove(path)
    return mods


def yaw_pose(yaw, t):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0, t[0]], [s, c, 0.0, t[1]], [0.0, 0.0, 1.0, t[2]]], np.float64)


def global_dicts(boxes, scores, labels, names, pose):
    """the dict list of waymo_tracking/test.py:212-256 from the f32 list rows (f64 from here on)"""
    xyz = boxes[:, :3].astype(np.float64)
    vel = np.concatenate([boxes[:, 6:8].astype(np.float64), np.zeros((len(boxes), 1))], 1)
    if pose is not None:
        xyz = np.einsum("ij,nj->ni", pose[:, :3], xyz) + pose[None, :, 3]
        vel = np.einsum("ij,nj->ni", pose[:, :3], vel)
    return [dict(translation=xyz[i], velocity=vel[i, :2], detection_name=names[int(labels[i])], score=scores[i], box_id=i)
            for i in range(len(boxes))]


def violations(tracker, dets, tracking_names, max_dist, lag, margin):
    """indices of dets whose decisions against tracker.tracks are closer than `margin` (f64)"""
    bad = []
    for i, d in enumerate(dets):
        if d["detection_name"] not in tracking_names:
            continue
        cls = tracking_names.index(d["detection_name"])
        q = np.asarray(d["translation"][:2], np.float64) + np.asarray(d["velocity"][:2], np.float64) * -1 * lag
        dist = np.array([np.hypot(*(t["ct"] - q)) for t in tracker.tracks if t["label_preds"] == cls], np.float64)
        md = max_dist[d["detection_name"]]
        valid = np.sort(dist[dist < md])
        if (np.abs(dist - md) < margin).any() or (len(valid) > 1 and valid[1] - valid[0] < margin):
            bad.append(i)
    return bad


def run_sequence(rng, tracker, names, tracking_names, max_dist, lag, n_obj, n_fp, first, empty=(), ego=None, low_scores=False):
    origin = np.zeros(2) if ego is None else np.array(ego["start"][:2])
    pos = origin + rng.uniform(-40, 40, (n_obj, 2))
    vel = rng.normal(0, 3, (n_obj, 2))
    cls = rng.integers(0, len(names), n_obj)
    inp = dict(boxes=np.zeros((FRAMES, CAP, 9), np.float32), scores=np.zeros((FRAMES, CAP), np.float32), labels=np.zeros((FRAMES, CAP), np.int64),
               count=np.zeros(FRAMES, np.int32), time_lag=np.zeros(FRAMES, np.float64), first=np.asarray(first, np.int32))
    if ego is not None:
        inp["pose"] = np.zeros((FRAMES, 3, 4), np.float64)
    tables, id_counts, redrawn = [], [], 0
    for f in range(FRAMES):
        dt = 0.0 if first[f] else lag
        pos = pos + vel * dt
        pose = None
        if ego is not None:
            pose = yaw_pose(ego["yaw"] + ego["yaw_rate"] * f, np.array(ego["start"]) + np.array(ego["vel"]) * lag * f)
            inp["pose"][f] = pose
        if first[f]:
            tracker.reset()
        seen = np.nonzero(rng.uniform(0, 1, n_obj) < 0.85)[0]
        n = 0 if f in empty else len(seen) + n_fp
        assert n <= CAP
        order = rng.permutation(n)
        margin = 1e-3 if ego is None else 8 * float(np.spacing(np.float32(np.abs(np.array(ego["start"])).max() + 100)))
        g_pos = np.concatenate([pos[seen], origin + rng.uniform(-40, 40, (n_fp, 2))])[:n] + rng.normal(0, 0.05, (n, 2))
        g_vel = np.concatenate([vel[seen], rng.normal(0, 3, (n_fp, 2))])[:n] + rng.normal(0, 0.2, (n, 2))
        labels = np.concatenate([cls[seen], rng.integers(0, len(names), n_fp)])[:n][order]
        z = rng.normal(-1, 0.3, n)
        scores = (np.clip(rng.normal(0.8, 0.15, n), 0.05, 0.99) if low_scores else rng.uniform(0.1, 0.99, n)).astype(np.float32)
        for attempt in range(200):
            boxes = np.zeros((n, 9), np.float64)
            if pose is None:
                boxes[:, :2], boxes[:, 6:8] = g_pos, g_vel
            else:                           # into the lidar frame: R^T (p - t), R^T v
                rot = pose[:2, :2]
                boxes[:, :2], boxes[:, 6:8] = (g_pos - pose[None, :2, 3]) @ rot, g_vel @ rot
            boxes[:, 2], boxes[:, 3:6], boxes[:, 8] = z, (1.9, 4.5, 1.6), 0.3
            boxes = boxes[order].astype(np.float32)
            dets = global_dicts(boxes, scores, labels, names, pose)
            bad = violations(tracker, dets, tracking_names, max_dist, dt, margin)
            if not bad:
                break
            redo = order[bad]               # list row i is object order[i]: new noise for the objects that violate a margin
            g_pos[redo] += rng.normal(0, 0.05, (len(redo), 2))
            redrawn += len(bad)
        else:
            raise AssertionError("no draw satisfies the decision margins")
        inp["boxes"][f, :n], inp["scores"][f, :n], inp["labels"][f, :n], inp["count"][f], inp["time_lag"][f] = boxes, scores, labels, n, dt
        ret = tracker.step_centertrack(dets, dt)
        assert ret is tracker.tracks or n == 0
        tables.append([dict(ct=np.asarray(t["ct"], np.float64), tracking=np.asarray(t["tracking"], np.float64), label=t["label_preds"],
                            tracking_id=t["tracking_id"], age=t["age"], active=t["active"], box_id=t["box_id"] if t["active"] > 0 else -1)
                       for t in tracker.tracks])
        id_counts.append(tracker.id_count)
    tm = max(len(t) for t in tables)
    out = dict(inp)
    for k, dt_, tail in (("ct", np.float64, (2,)), ("tracking", np.float64, (2,)), ("label", np.int32, ()), ("tracking_id", np.int32, ()),
                         ("age", np.int32, ()), ("active", np.int32, ()), ("box_id", np.int32, ())):
        a = np.zeros((FRAMES, tm) + tail, dt_)
        for f, t in enumerate(tables):
            if t:
                a[f, :len(t)] = np.array([row[k] for row in t], dt_)
        out["t_" + k] = a
    out["t_count"] = np.array([len(t) for t in tables], np.int32)
    out["id_count"] = np.array(id_counts, np.int32)
    return out, redrawn


def main():
    nusc, waymo = reference_trackers()
    r = np.random.default_rng(20)
    out = {}
    styles = {
        "nusc": (NUSC_CLASSES, list(nusc.NUSCENES_TRACKING_NAMES), dict(nusc.NUSCENE_CLS_VELOCITY_ERROR), -np.inf, 0.5),
        "waymo": (WAYMO_CLASSES, list(waymo.WAYMO_TRACKING_NAMES), WAYMO_MAX_DIST, 0.75, 0.1),
    }
    for style, (names, tnames, md, thresh, lag) in styles.items():
        out[f"{style}_class_names"], out[f"{style}_tracking_names"] = np.array(names), np.array(tnames)
        out[f"{style}_track_class"] = np.array([tnames.index(n) if n in tnames else -1 for n in names], np.int32)
        out[f"{style}_max_dist"] = np.array([md.get(n, 0.0) for n in names], np.float32)
        out[f"{style}_max_age"], out[f"{style}_score_thresh"] = np.int32(3), np.float32(thresh)
    ego = dict(start=(3150.0, -2240.0, 12.0), vel=(9.0, 4.0, 0.0), yaw=0.7, yaw_rate=0.04)
    start = [1] + [0] * (FRAMES - 1)
    cases = {
        "nusc_a": dict(style="nusc", n_obj=44, n_fp=4, first=start),
        "nusc_b": dict(style="nusc", n_obj=24, n_fp=2, first=[1, 0, 0, 1, 0, 0, 0, 0], empty=(5,)),
        "waymo_a": dict(style="waymo", n_obj=40, n_fp=3, first=start, low_scores=True),
        "waymo_b": dict(style="waymo", n_obj=28, n_fp=2, first=start, ego=ego, low_scores=True),
    }
    for tag, c in cases.items():
        names, tnames, md, thresh, lag = styles[c.pop("style")]
        tracker = nusc.PubTracker(hungarian=False, max_age=3) if tag.startswith("nusc") else \
            waymo.PubTracker(max_age=3, max_dist=md, score_thresh=thresh)
        res, redrawn = run_sequence(r, tracker, names, tnames, md, lag, **c)
        for k, v in res.items():
            out[f"{tag}_{k}"] = v
        coast = int(((res["t_active"] == 0) & (np.arange(res["t_active"].shape[1])[None] < res["t_count"][:, None])).sum())
        print(tag, "counts", res["count"].tolist(), "table", res["t_count"].tolist(), "ids", int(res["id_count"][-1]), "coasting rows", coast,
              "longest active", int(res["t_active"].max()), "redrawn", redrawn)
        assert coast > 0 and res["t_active"].max() >= 3
    path = os.path.join(HERE, "track.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote track.npz %8.1f KB" % (size / 1024))
    assert size < 100 * 1024


if __name__ == "__main__":
    main()
