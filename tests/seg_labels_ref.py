"""numpy restatement of the seg super-task's label builders, written from their semantics (not from the reference's loops):

``voxel_labels_vote``: per grid cell the majority vote of its points' labels.  A point votes when its label is in [0, 255] and it has
a cell (every grid index inside the grid); the winner has the most votes, the lowest label among equals; label 0 votes like any other,
so a cell that 0 wins -- like a cell without voters -- holds 0.  Counts are exact (the reference's uint16 counters wrap at 65536) and
labels above 255 do not vote (the reference raises IndexError).

``pool_labels``: per window of (kh, kw, kl) cells the most frequent label among 1..255 minus one, the lowest among equals, -1 for a
window without one; trailing planes / rows / columns that do not fill a window are dropped.
"""
import numpy as np

LABEL_SLOTS = 256


def voxel_labels_vote(grid_ind: np.ndarray, point_labels: np.ndarray, batch: int, grid_zyx) -> np.ndarray:
    """grid_ind (N, 4) rows [b, z, y, x], point_labels (N,) integer -> voxel_labels (batch, Z, H, W) int64"""
    z, h, w = (int(v) for v in grid_zyx)
    gi = np.asarray(grid_ind, dtype=np.int64).reshape(-1, 4)
    lab = np.asarray(point_labels).reshape(-1).astype(np.int64)
    assert gi.shape[0] == lab.shape[0]
    inside = (gi >= 0).all(1) & (gi[:, 0] < batch) & (gi[:, 1] < z) & (gi[:, 2] < h) & (gi[:, 3] < w)
    votes = inside & (lab >= 0) & (lab < LABEL_SLOTS)
    cell = ((gi[votes, 0] * z + gi[votes, 1]) * h + gi[votes, 2]) * w + gi[votes, 3]
    out = np.zeros(batch * z * h * w, np.int64)
    if cell.size:
        cells, inv = np.unique(cell, return_inverse=True)
        counts = np.zeros((len(cells), LABEL_SLOTS), np.int64)
        np.add.at(counts, (inv.reshape(-1), lab[votes]), 1)
        out[cells] = counts.argmax(1)               # first maximum: the lowest label among equals
    return out.reshape(batch, z, h, w)


def loss_labels(voxel_labels: np.ndarray) -> np.ndarray:
    """what SegLoss takes: (cells,) int32 holding label - 1, -1 where the cell is unlabelled"""
    return (voxel_labels.reshape(-1) - 1).astype(np.int32)


def pool_labels(labels: np.ndarray, kh: int, kw: int, kl: int) -> np.ndarray:
    """labels (B, Z, H, W) integer -> (B, Z // kh, H // kw, W // kl) int64"""
    lab = np.asarray(labels).astype(np.int64)
    b, z, h, w = lab.shape
    zo, ho, wo = z // kh, h // kw, w // kl
    win = lab[:, :zo * kh, :ho * kw, :wo * kl].reshape(b, zo, kh, ho, kw, wo, kl).transpose(0, 1, 3, 5, 2, 4, 6).reshape(b, zo, ho, wo, -1)
    counts = np.zeros((b, zo, ho, wo, LABEL_SLOTS), np.int64)
    for k in range(win.shape[-1]):
        v = win[..., k]
        ok = (v >= 1) & (v < LABEL_SLOTS)
        idx = np.nonzero(ok)
        np.add.at(counts, idx + (v[ok],), 1)
    best = counts[..., 1:].argmax(-1)               # index c <-> label c + 1; first maximum
    return np.where(counts[..., 1:].sum(-1) > 0, best, -1).astype(np.int64)


def get_labels(labels: np.ndarray, pred_shape) -> np.ndarray:
    """the label helper of the seg head on (B,H,W) or (B,Z,H,W) labels: equal shapes -> labels - 1, otherwise the pooled labels with
    floor-division factors (kh = Z against a 2-D prediction); a single output plane is dropped"""
    label_shape, pred_shape = tuple(labels.shape[1:]), tuple(pred_shape)
    if label_shape == pred_shape:
        return labels - 1
    kw, kl = label_shape[-2] // pred_shape[-2], label_shape[-1] // pred_shape[-1]
    kh = 1 if len(label_shape) == 2 else (label_shape[0] if len(pred_shape) == 2 else label_shape[0] // pred_shape[0])
    out = pool_labels(labels if labels.ndim == 4 else labels[:, None], kh, kw, kl)
    return out[:, 0] if out.shape[1] == 1 else out
