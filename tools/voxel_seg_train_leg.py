#!/usr/bin/env python3
"""Training the voxel-wise segmentation head alone at the shape of tools/voxel_seg_leg.py: B = 1, a 640 x 640 x 40 grid
with 100 k active voxels (the same seeded clustered columns), the 80 x 80 x 512 neck map, and about as many labelled cells as voxels: nine
in ten voxels and a tenth as many cells that hold no voxel.  Device events, warmed, `--reps` launches per event pair, `--rounds` pairs,
medians with min-max.

Prints the time of every NEW launch (the labelled-cell list, the query index, the three backward kernels, the overlap-add's adjoint), of the
head's forward at the labelled cells and the loss, and of head forward + loss + backward on the tape, each new launch beside its BOUND: the
larger of its FLOP over the 157.3 TFLOP/s f32 peak and its bytes over the 8 TB/s HBM peak, counted from the shapes and the seeded
occupancy by the code below (the least the hardware could take, not a prediction).

    python tools/voxel_seg_train_leg.py [--voxels 100000] [--reps 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from partner_amd import autodiff as ad  # noqa: E402
from partner_amd import hip, ops  # noqa: E402
from partner_amd.seg_heads import DeconvConvHead, seg_loss_nhwc  # noqa: E402
from partner_amd.train_voxel_seg import voxel_seg_head_train  # noqa: E402
from voxel_seg_leg import CIN, CV, D, H, NC, PEAK_BYTES, PEAK_FLOPS, S, W, draw_voxels  # noqa: E402


def counts(cells, q):
    """FLOP and bytes of every new launch from the shapes and the occupancy; q: the labelled cells [z, y, x]"""
    ncp, slabs, nq, v = 16, D + (D + 15) // 16, len(q), len(cells)
    occ = np.zeros((H + 2, W + 2), np.int64)
    np.add.at(occ, (cells[:, 1] + 1, cells[:, 2] + 1), 1)
    box = sum(occ[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    nbrs = int(box[q[:, 1], q[:, 2]].sum())                               # (query, active neighbour) pairs
    qocc = np.zeros((H + 2, W + 2), np.int64)
    np.add.at(qocc, (q[:, 1] + 1, q[:, 2] + 1), 1)
    qbox = sum(qocc[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    pairs_u = int(qbox.sum())                                             # (pixel, query in its window) pairs
    wbytes = 4.0 * D * slabs * 9 * 16 * ncp
    m, n_gemm = (H // S) * (W // S), 4 * S * S * D
    out = {
        "label_queries": dict(flop=0.0, bytes=2.0 * H * W * D + 8.0 * nq),
        "query_index": dict(flop=0.0, bytes=16.0 * nq + 8.0 * ((H * W * D + 31) // 32) * 2),
        "wgrad": dict(flop=2.0 * NC * (CV * nbrs + 9.0 * D * nq), bytes=wbytes + 4.0 * (nq * ncp + v * CV + nq * 9 * D)),
        "dfeat": dict(flop=2.0 * NC * CV * nbrs, bytes=wbytes + 4.0 * (nq * ncp + v * CV)),
        "du": dict(flop=2.0 * NC * D * pairs_u, bytes=wbytes + 4.0 * (nq * ncp + H * W * D)),
        "overlap_bwd": dict(flop=0.0, bytes=4.0 * (m * n_gemm + H * W * D)),
    }
    for k in out.values():
        t_f, t_b = k["flop"] / PEAK_FLOPS, k["bytes"] / PEAK_BYTES
        k["bound_us"] = round(max(t_f, t_b) * 1e6, 2)
        k["bound_by"] = "flop" if t_f > t_b else "bytes"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    hip.load()
    dev = torch.device("cuda:0")
    g = np.random.Generator(np.random.PCG64(2024))
    cells = draw_voxels(a.voxels, g)
    v = len(cells)
    feats = np.abs(g.standard_normal((v, CV))).astype(np.float32)
    x2 = g.standard_normal((1, H // S, W // S, CIN)).astype(np.float32)
    lab = np.zeros((1, D, H, W), np.uint8)
    keep = cells[g.random(v) < 0.9]
    lab[0, keep[:, 0], keep[:, 1], keep[:, 2]] = g.integers(1, NC + 1, len(keep))
    off = cells[g.integers(0, v, v // 10)].copy()                          # a tenth as many cells moved along z: mostly no voxel there
    off[:, 0] = (off[:, 0] + g.integers(1, D, len(off))) % D
    lab[0, off[:, 0], off[:, 1], off[:, 2]] = g.integers(1, NC + 1, len(off))
    q = np.argwhere(lab[0] > 0)
    cap = len(q) + 4096
    head = DeconvConvHead(kernel=3, num_classes=NC, in_channels_voxel=CV, in_channels=CIN, up_scale=S, height=D)
    with torch.no_grad():
        head.deconv.weight.copy_(torch.from_numpy((g.standard_normal(tuple(head.deconv.weight.shape)) / np.sqrt(CIN)).astype(np.float32)))
        head.conv.weight.copy_(torch.from_numpy((g.standard_normal(tuple(head.conv.weight.shape)) / np.sqrt(9.0 * D * 3)).astype(np.float32)))
        head.conv.bias.copy_(torch.from_numpy((0.1 * g.standard_normal(NC * D)).astype(np.float32)))
    head = head.to(dev).train()

    import ctypes as C
    dims = [1, D, H, W]
    coors = torch.from_numpy(np.concatenate([np.zeros((v, 1), np.int64), cells], 1).astype(np.int32)).to(dev)
    index = torch.empty(hip.load().pn_sparse_index_bytes(D * H * W), dtype=torch.uint8, device=dev)
    keys, rank = torch.empty(v, dtype=torch.int32, device=dev), torch.empty(v, dtype=torch.int32, device=dev)
    count, n_dev = torch.empty(1, dtype=torch.int32, device=dev), torch.full((1,), v, dtype=torch.int32, device=dev)
    hip.call("pn_sparse_index_from_coords", coors.data_ptr(), v, n_dev.data_ptr(), (C.c_int32 * 4)(*dims), index.data_ptr(), keys.data_ptr(), count.data_ptr(),
             rank.data_ptr(), hip.stream())
    level = ops.SparseLevel(feats=torch.from_numpy(feats).to(dev), index=index, keys=keys, count=count, cap=v, dims=dims)
    x2d, labd = torch.from_numpy(x2).to(dev), torch.from_numpy(lab).to(dev)

    qk, qlab, qn, _ = ops.voxel_seg_label_queries(labd, NC, cap)
    packed, pbias = ops.voxel_seg_pack(head.conv.weight, head.conv.bias, D, NC)
    u = ops.DeconvOverlap(head.deconv.weight, S)(x2d)
    logits = torch.zeros((cap, 16), dtype=torch.float32, device=dev)
    ops.voxel_seg_logits(level, u, packed, pbias, NC, qk, qn, out=logits)
    _, dl, _ = seg_loss_nhwc(logits, 16, NC, qlab, -1, max_valid=cap)
    qindex = ops.voxel_seg_query_index(qk, qn, dims)
    d_u = ops.voxel_seg_du(dims, qindex, dl, packed, NC)

    def whole():
        t = ad.Tape()
        c1, xn = t.input(level.feats), t.input(x2d)
        k2, l2, n2, _ = ops.voxel_seg_label_queries(labd, NC, cap)
        lg = voxel_seg_head_train(t, head, c1, level, xn, k2, n2)
        _, g2, _ = seg_loss_nhwc(lg.v, 16, NC, l2, -1, max_valid=cap)
        ad.accumulate(lg, g2)
        t.backward()

    fns = dict(label_queries=lambda: ops.voxel_seg_label_queries(labd, NC, cap),
               logits_fwd=lambda: ops.voxel_seg_logits(level, u, packed, pbias, NC, qk, qn, out=logits),
               seg_loss=lambda: seg_loss_nhwc(logits, 16, NC, qlab, -1, max_valid=cap),
               query_index=lambda: ops.voxel_seg_query_index(qk, qn, dims),
               wgrad=lambda: ops.voxel_seg_wgrad(level, u, qk, qn, dl, NC),
               dfeat=lambda: ops.voxel_seg_dfeat(level, qindex, dl, packed, NC),
               du=lambda: ops.voxel_seg_du(dims, qindex, dl, packed, NC),
               overlap_bwd=lambda: ops.deconv_overlap_bwd(d_u, S),
               head_fwd_loss_bwd=whole)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps       # us per call

    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, a.reps))
    bounds = counts(cells, q)
    vox = np.zeros((D, H, W), bool)
    vox[cells[:, 0], cells[:, 1], cells[:, 2]] = True
    res = dict(voxels=v, labelled_cells=int(len(q)), labelled_cells_without_a_voxel=int((~vox[q[:, 0], q[:, 1], q[:, 2]]).sum()), capacity=cap)
    for k in fns:
        res[k + "_us"] = round(statistics.median(t[k]), 2)
        res[k + "_us_min_max"] = [round(min(t[k]), 2), round(max(t[k]), 2)]
        if k in bounds:
            res[k + "_bound"] = bounds[k]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
