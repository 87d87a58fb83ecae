"""Center-based tracking on the device: the consumer of ``CenterHead.predict(device_only=True)``.

The reference ships, beside every CenterPoint-family detector, the tracker that turns its velocity outputs into tracks
(tools/nusc_tracking/pub_tracker.py with track_utils.py, tools/waymo_tracking/tracker.py, driven by tools/waymo_tracking/test.py and
tools/nusc_tracking/pub_test.py): Python loops over an N x M matrix on the host.  Here one HIP launch per frame (`pn_track_step_f32`,
csrc/track.hip) does the same greedy association on the device list, one block per sequence, with nothing read back; the track table lives
in one device blob that is updated in place, so a step can be captured in a hipGraph.

``DeviceTracker`` is the device API; ``PubTracker`` / ``WaymoPubTracker`` keep the reference's ``step_centertrack(results, time_lag)`` over
lists of dicts and run the same kernel.  The one deliberate difference from the reference: a non-empty list whose rows are ALL of
untracked classes raises IndexError there (``results[0]``); here the tracks coast.  As everywhere in this package there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import hip
from .hip import PartnerHipError

# tools/nusc_tracking/pub_tracker.py:8-30
NUSCENES_TRACKING_NAMES = ["bicycle", "bus", "car", "motorcycle", "pedestrian", "trailer", "truck"]
NUSCENE_CLS_VELOCITY_ERROR = {"car": 4, "truck": 4, "bus": 5.5, "trailer": 3, "pedestrian": 1, "motorcycle": 13, "bicycle": 3}
# tools/waymo_tracking/tracker.py:21-25
WAYMO_TRACKING_NAMES = ["VEHICLE", "PEDESTRIAN", "CYCLIST"]

_LIST_KEYS = ("box3d_lidar", "scores", "label_preds", "count")
_F64_COLS = ("ct", "tracking")
_I32_COLS = ("label", "tracking_id", "age", "active", "box_id")


class DeviceTracker:
    """Greedy center-based tracker of ``batch`` independent sequences over device detection lists of ``capacity`` rows.

    class_names     the detector's class list: ``label_preds`` indexes it
    tracking_names  the classes that are tracked, in the order that defines the tracks' ``label_preds`` (tracker.py:56)
    max_dist        {tracking name: metres}: a detection further than this from a track's centre does not match it (tracker.py:76, :86)
    max_age         a track unseen for this many frames is dropped; 0 = nothing coasts
    score_thresh    an unmatched detection starts a track only when score > score_thresh (tracker.py:113); None = always (nuScenes)
    """

    def __init__(self, class_names: Sequence[str], tracking_names: Sequence[str], max_dist: Dict[str, float], max_age: int = 0,
                 score_thresh: Optional[float] = None, batch: int = 1, capacity: int = 500, device=None):
        self.class_names, self.tracking_names = list(class_names), list(tracking_names)
        missing = [n for n in self.tracking_names if n in self.class_names and n not in max_dist]
        if missing:
            raise ValueError(f"DeviceTracker: max_dist names no distance for the tracked classes {missing}")
        self.max_age, self.batch, self.capacity = int(max_age), int(batch), int(capacity)
        self.score_thresh = -math.inf if score_thresh is None else float(score_thresh)
        self.rows = self.capacity * max(1, self.max_age)
        lib = hip.load()
        nbytes = int(lib.pn_track_state_bytes(self.batch, self.capacity, self.max_age))
        if nbytes == 0:
            raise ValueError(f"DeviceTracker: batch {batch}, capacity {capacity}, max_age {max_age} is outside what pn_track_step_f32 takes "
                             "(capacity <= 4096, T = capacity * max(1, max_age) <= 8192, 12 T + 28 capacity <= 64512 bytes of LDS)")
        self.device, self.state, self.tracks = (None if device is None else torch.device(device)), None, None
        if self.device is not None and self.device.type != "cuda":
            raise PartnerHipError("DeviceTracker runs only on a gfx950 (MI355X) device through libpartner_hip.so; there is deliberately no CPU fallback")
        self._state_bytes = nbytes
        self._track_class = [self.tracking_names.index(n) if n in self.tracking_names else -1 for n in self.class_names]
        self._max_dist = [float(max_dist[n]) if n in self.tracking_names else 0.0 for n in self.class_names]

    def _allocate(self, dev) -> None:
        """state, tables and outputs on the device of the first list (or the one named at construction)"""
        self.device = dev
        self.track_class = torch.tensor(self._track_class, dtype=torch.int32, device=dev)
        self.max_dist = torch.tensor(self._max_dist, dtype=torch.float32, device=dev)
        # the blob of pn_track_state_bytes (layout: include/partner_hip.h); float64 storage keeps it 8-byte aligned
        self.state = torch.zeros((self._state_bytes + 7) // 8, dtype=torch.float64, device=dev)
        bt, i32 = self.batch * self.rows, self.state.view(torch.int32)
        self.tracks = {k: self.state[2 * bt * j:2 * bt * (j + 1)].view(self.batch, self.rows, 2) for j, k in enumerate(_F64_COLS)}
        for j, k in enumerate(_I32_COLS):
            self.tracks[k] = i32[16 * bt + bt * j:16 * bt + bt * (j + 1)].view(self.batch, self.rows)
        self.tracks["track_count"] = i32[24 * bt:24 * bt + self.batch]
        self.tracks["id_count"] = i32[24 * bt + self.batch:24 * bt + 2 * self.batch]
        self.tracking_ids = torch.zeros((self.batch, self.capacity), dtype=torch.int32, device=dev)
        self.active = torch.zeros((self.batch, self.capacity), dtype=torch.int32, device=dev)
        self._zero_first = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        self.reset()

    @classmethod
    def nuscenes(cls, class_names, max_age=3, **kw):
        """tools/nusc_tracking/pub_tracker.py: its tracking names and NUSCENE_CLS_VELOCITY_ERROR; every unmatched detection starts a track"""
        return cls(class_names, NUSCENES_TRACKING_NAMES, NUSCENE_CLS_VELOCITY_ERROR, max_age=max_age, score_thresh=None, **kw)

    @classmethod
    def waymo(cls, max_age=3, vehicle=0.8, pedestrian=0.4, cyclist=0.6, score_thresh=0.75, class_names=None, **kw):
        """the defaults of tools/waymo_tracking/test.py:34-38 (label_to_name :185-193 is the class list)"""
        return cls(WAYMO_TRACKING_NAMES if class_names is None else class_names, WAYMO_TRACKING_NAMES,
                   {"VEHICLE": vehicle, "PEDESTRIAN": pedestrian, "CYCLIST": cyclist}, max_age=max_age, score_thresh=score_thresh, **kw)

    def reset(self) -> None:
        """every sequence: empty table, id_count 0 (PubTracker.reset); one sequence alone is reset by its ``first`` flag"""
        if self.state is not None:
            self.state.zero_()
            self.tracks["box_id"].fill_(-1)

    def _check_list(self, det_list):
        if not isinstance(det_list, dict) or any(k not in det_list for k in _LIST_KEYS):
            raise TypeError("DeviceTracker.step: det_list must be the dict predict(device_only=True) returns "
                            f"(keys {', '.join(_LIST_KEYS)})")
        boxes, scores, labels, count = (det_list[k] for k in _LIST_KEYS)
        if not all(isinstance(t, torch.Tensor) for t in (boxes, scores, labels, count)):
            raise TypeError("DeviceTracker.step: det_list must hold tensors (the device_only dict)")
        if boxes.dim() != 3 or boxes.shape[-1] != 9:
            raise ValueError(f"DeviceTracker.step: box3d_lidar has shape {tuple(boxes.shape)}; center-based tracking needs the 9-column boxes "
                             "(x, y, z, w, l, h, vx, vy, rot): a 7-column list has no velocity")
        hip.require_device(boxes, scores, labels, count)
        b, cap = self.batch, self.capacity
        for name, t, shape, dt in (("box3d_lidar", boxes, (b, cap, 9), torch.float32), ("scores", scores, (b, cap), torch.float32),
                                   ("label_preds", labels, (b, cap), torch.int64), ("count", count, (b,), torch.int32)):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"DeviceTracker.step: det_list['{name}'] must be a contiguous {shape} {dt} tensor, got {tuple(t.shape)} {t.dtype}")
        return boxes, scores, labels, count

    def _per_sequence(self, value, name, dtype, shape):
        if isinstance(value, torch.Tensor):
            hip.require_device(value)
            if tuple(value.shape) != shape or value.dtype != dtype or not value.is_contiguous():
                raise ValueError(f"DeviceTracker.step: {name} must be a contiguous {shape} {dtype} tensor, got {tuple(value.shape)} {value.dtype}")
            return value
        host = torch.as_tensor(np.broadcast_to(np.asarray(value, dtype=np.float64 if dtype == torch.float64 else np.int32), shape).copy())
        return host.to(self.device)

    def step(self, det_list, time_lag, pose=None, first=None):
        """One frame for every sequence.  ``time_lag`` (B,) f64 seconds since the sequence's previous frame, ``pose`` (B, 3, 4) f64 lidar ->
        tracking frame (None: the list is global already), ``first`` (B,) int32, nonzero = reset that sequence first.  Device tensors are
        used as they are -- nothing synchronises, the call is capturable --; Python values / arrays are uploaded.  Returns
        {'tracking_ids', 'active': (B, cap) int32 aligned with the list rows, 0 = no track; 'tracks': views of the state: 'ct', 'tracking'
        (B, T, 2) f64, 'label', 'tracking_id', 'age', 'active', 'box_id' (B, T) int32, 'track_count', 'id_count' (B,)}: the same tensors
        every call."""
        boxes, scores, labels, count = self._check_list(det_list)
        if self.state is None:
            self._allocate(boxes.device if self.device is None else self.device)
        b = self.batch
        lag = self._per_sequence(time_lag, "time_lag", torch.float64, (b,))
        pose_t = None if pose is None else self._per_sequence(pose, "pose", torch.float64, (b, 3, 4))
        first_t = self._zero_first if first is None else self._per_sequence(first, "first", torch.int32, (b,))
        hip.call("pn_track_step_f32", hip.ptr(boxes), 9, hip.ptr(scores), hip.ptr(labels), hip.ptr(count), hip.ptr(pose_t), hip.ptr(lag),
                 hip.ptr(first_t), hip.ptr(self.track_class), hip.ptr(self.max_dist), len(self.class_names), self.max_age,
                 C.c_float(self.score_thresh), b, self.capacity, hip.ptr(self.state), hip.ptr(self.tracking_ids), hip.ptr(self.active),
                 hip.stream())
        return {"tracking_ids": self.tracking_ids, "active": self.active, "tracks": self.tracks}

    def to_host(self, out, det_list=None) -> List[Dict[str, np.ndarray]]:
        """ONE readback.  Per sequence the reference's output list in the reference's order, i.e. the table rows with active > 0 -- what
        waymo_tracking/test.py:117-141 consumes --: 'box_id' (rows of this frame's list), 'tracking_id', 'active', 'label_preds' (index in
        the tracking names), 'ct'; with ``det_list`` also the list rows themselves, 'box3d_lidar' and 'scores' at box_id (test.py:135-141)."""
        t = out["tracks"]
        cols = [t["ct"].reshape(self.batch, -1), t["label"].double(), t["tracking_id"].double(), t["active"].double(), t["box_id"].double(),
                t["track_count"].double().unsqueeze(1)]
        if det_list is not None:
            cols += [det_list["box3d_lidar"].reshape(self.batch, -1).double(), det_list["scores"].double()]
        flat = torch.cat(cols, 1).cpu().numpy()          # int32 and f32 are exact in f64
        rows, res = self.rows, []
        for b in range(self.batch):
            f = flat[b]
            n = int(f[6 * rows])
            sel = np.nonzero(f[4 * rows:4 * rows + n] > 0)[0]
            d = dict(ct=f[:2 * rows].reshape(rows, 2)[sel], label_preds=f[2 * rows:3 * rows][sel].astype(np.int32),
                     tracking_id=f[3 * rows:4 * rows][sel].astype(np.int32), active=f[4 * rows:5 * rows][sel].astype(np.int32),
                     box_id=f[5 * rows:6 * rows][sel].astype(np.int32))
            if det_list is not None:
                o = 6 * rows + 1
                boxes = f[o:o + 9 * self.capacity].reshape(self.capacity, 9).astype(np.float32)
                d["box3d_lidar"] = boxes[d["box_id"]]
                d["scores"] = f[o + 9 * self.capacity:o + 10 * self.capacity].astype(np.float32)[d["box_id"]]
            res.append(d)
        return res


class _HostFrontEnd:
    """``step_centertrack(results, time_lag)`` of the reference over its lists of dicts, on the kernel.  The dicts are uploaded as a
    global-frame list (identity pose) of float32 rows: a ``translation`` or ``velocity`` that float32 cannot hold exactly is ROUNDED by the
    upload (the reference keeps them in float64).  For large global coordinates use ``DeviceTracker`` with the lidar-frame list and an f64
    ``pose``, which is what keeps f64 centres.  The device table grows with the longest list seen (it is rebuilt, tracks kept)."""

    _tracking_names: List[str] = []

    def __init__(self, max_dist, max_age, score_thresh):
        self.max_age, self._max_dist, self._score_thresh = max_age, dict(max_dist), score_thresh
        self._tracker: Optional[DeviceTracker] = None
        self.reset()

    def reset(self):
        self.id_count = 0
        self.tracks: List[dict] = []
        if self._tracker is not None:
            self._tracker.reset()

    def _ensure(self, n):
        old = self._tracker
        if old is not None and old.capacity >= n:
            return
        cap = max(64, 1 << (max(n, 1) - 1).bit_length())
        new = DeviceTracker(self._tracking_names, self._tracking_names, self._max_dist, max_age=self.max_age, score_thresh=self._score_thresh,
                            batch=1, capacity=cap)
        if old is not None and old.state is not None:
            new._allocate(old.device)                     # carry the table over: the columns keep their order, only the row count grows
            for k in _F64_COLS + _I32_COLS:
                new.tracks[k][:, :old.rows] = old.tracks[k]
            new.tracks["track_count"].copy_(old.tracks["track_count"])
            new.tracks["id_count"].copy_(old.tracks["id_count"])
        self._tracker = new

    def step_centertrack(self, results, time_lag):
        if len(results) == 0:                     # tracker.py:43-45
            self.tracks = []
            if self._tracker is not None and self._tracker.state is not None:
                self._tracker.tracks["track_count"].zero_()
            return []
        names = self._tracking_names
        kept = [d for d in results if d["detection_name"] in names]
        if not kept:
            raise IndexError("step_centertrack: every detection is of a class that is not tracked (the reference fails at results[0])")
        self._ensure(len(kept))
        trk = self._tracker
        cap = trk.capacity
        host = np.zeros((cap, 11), np.float32)
        for i, d in enumerate(kept):
            d["ct"], d["tracking"] = np.array(d["translation"][:2]), np.array(d["velocity"][:2]) * -1 * time_lag      # tracker.py:54-56
            d["label_preds"] = names.index(d["detection_name"])
            host[i, 0:2], host[i, 6:8] = d["translation"][:2], d["velocity"][:2]
            host[i, 9], host[i, 10] = d["score"], names.index(d["detection_name"])
        dev = torch.from_numpy(host).to(trk.device if trk.device is not None else torch.device("cuda", torch.cuda.current_device()))
        det_list = dict(box3d_lidar=dev[:, :9].contiguous().view(1, cap, 9), scores=dev[:, 9].contiguous().view(1, cap),
                        label_preds=dev[:, 10].to(torch.int64).view(1, cap),
                        count=torch.tensor([len(kept)], dtype=torch.int32, device=dev.device))
        out = trk.step(det_list, float(time_lag))
        t = out["tracks"]
        flat = torch.cat([t["ct"].reshape(1, -1), t["tracking"].reshape(1, -1)] + [t[k].double() for k in _I32_COLS]
                         + [t["track_count"].double().view(1, 1), t["id_count"].double().view(1, 1)], 1).cpu().numpy()[0]
        rows = trk.rows
        ct, tracking = flat[:2 * rows].reshape(rows, 2), flat[2 * rows:4 * rows].reshape(rows, 2)
        label, tid, age, active, box_id = (flat[(4 + j) * rows:(5 + j) * rows].astype(np.int64) for j in range(5))
        count, self.id_count = int(flat[9 * rows]), int(flat[9 * rows + 1])
        by_id = {d["tracking_id"]: d for d in self.tracks}
        ret = []
        for r in range(count):
            if box_id[r] >= 0:                    # a detection of this frame: the caller's dict, augmented
                d = kept[box_id[r]]
            else:                                 # a coasting track: the dict it was last seen as
                d = by_id[int(tid[r])]
            d["ct"], d["tracking"], d["label_preds"] = ct[r].copy(), tracking[r].copy(), int(label[r])
            d["tracking_id"], d["age"], d["active"] = int(tid[r]), int(age[r]), int(active[r])
            ret.append(d)
        self.tracks = ret
        return ret


class PubTracker(_HostFrontEnd):
    """tools/nusc_tracking/pub_tracker.py:34-154 (greedy matching)"""

    _tracking_names = NUSCENES_TRACKING_NAMES

    def __init__(self, hungarian=False, max_age=0):
        if hungarian:
            raise NotImplementedError("PubTracker(hungarian=True): the reference's own branch calls linear_assignment, which it neither defines "
                                      "nor imports (pub_tracker.py:98); only the greedy matching exists")
        self.hungarian = False
        self.NUSCENE_CLS_VELOCITY_ERROR = NUSCENE_CLS_VELOCITY_ERROR
        super().__init__(NUSCENE_CLS_VELOCITY_ERROR, max_age, None)


class WaymoPubTracker(_HostFrontEnd):
    """tools/waymo_tracking/tracker.py:27-136"""

    _tracking_names = WAYMO_TRACKING_NAMES

    def __init__(self, max_age=0, max_dist={}, score_thresh=0.1):
        self.WAYMO_CLS_VELOCITY_ERROR = max_dist
        self.WAYMO_TRACKING_NAMES = WAYMO_TRACKING_NAMES
        self.score_thresh = score_thresh
        super().__init__(max_dist, max_age, score_thresh)
