#!/usr/bin/env python3
"""Golden-vector generator: runs the REFERENCE code (imported from /root/reference with
third-party stand-ins, see ref_import.py) on deterministic inputs and stores inputs that
cannot be re-created plus the reference's outputs as small ``.npz`` fixtures.

Container-only: ``python tests/golden/make_golden.py``.  The fixtures it writes are the
pins for ``oracle/`` (CPU restatement) and, through the oracle, for the HIP path.

Every weight tensor is produced by ``partner_amd.utils.synth.fill_state_dict`` (name-keyed
numpy RNG), every sweep by ``synth_sweep_*`` -- so the fixtures only need to hold outputs.
"""
from __future__ import annotations

import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_import  # noqa: E402
from partner_amd.utils import synth  # noqa: E402

torch.set_num_threads(8)
torch.manual_seed(0)
logging.basicConfig(level=logging.WARNING)

det3d = ref_import.import_reference()
from addict import Dict as ADict  # stub from ref_import  # noqa: E402
from det3d.datasets.pipelines.utils import transform_points  # noqa: E402
from det3d.datasets.pipelines.voxelization import Voxelization  # noqa: E402
from det3d.core.input.voxel_generator import VoxelGenerator  # noqa: E402
from det3d.torchie.parallel.collate import collate_kitti_one_sector  # noqa: E402
from det3d.models import build_detector  # noqa: E402
from det3d.models.readers.voxel_encoder import DynamicVoxelEncoderV1, VoxelFeatureExtractorV3  # noqa: E402
from det3d.models.readers.pillar_encoder import DynamicPFNet, DynamicPPScatter  # noqa: E402
from det3d.models.necks.rpn import RPN  # noqa: E402
from det3d.models.bbox_heads.center_head import CenterHead  # noqa: E402
from det3d.models.bbox_heads.center_head_parallel import CenterHeadSingle, CenterHeadSinglePos  # noqa: E402
from det3d.models.utils.set_transformer import SetBlock  # noqa: E402


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print("wrote %-28s %8.1f KB" % (name, os.path.getsize(path) / 1024))


def vox_cfg(rng_, vs, dynamic=True, max_points=20, max_voxels=(30000, 60000)):
    return ADict(range=list(rng_), voxel_size=list(vs), max_points_in_voxel=max_points,
                 max_voxel_num=list(max_voxels) if not isinstance(max_voxels, int) else max_voxels,
                 voxel_shape="cylinder", return_density=False, dynamic=dynamic, nsectors=1)


def ref_grid_ind(points, rng_, vs):
    v = Voxelization(cfg=vox_cfg(rng_, vs), super_tasks=["det"])
    res = {"mode": "val", "voxel_shape": "cylinder", "lidar": {"points": points}}
    res, _ = v.voxelize_dynamic(res, {})
    vox = res["lidar"]["voxels"]
    return vox["grid_ind"], vox["shape"], vox["range"], vox["size"]


def collate_grid_ind(list_of_gi):
    """Reference batch-index prepend (collate.py:157-164) via the reference's collate."""
    batch = [{"grid_ind": g, "metadata": i} for i, g in enumerate(list_of_gi)]
    return collate_kitti_one_sector(batch)["grid_ind"].numpy()


def edge_points(rng_, vs, grid, seed):
    """polar points (n,7) sitting exactly on bin edges, just inside/outside the range."""
    r = np.random.default_rng(seed)
    lo = np.asarray(rng_[:3], np.float32)
    vsz = np.asarray(vs, np.float32)
    rows = []
    for ax in range(3):
        ks = np.unique(np.concatenate([np.arange(0, min(grid[ax], 40)), grid[ax] - 1 - np.arange(0, min(grid[ax], 8)),
                                       r.integers(0, grid[ax], 40)]))
        for k in ks:
            edge = np.float32(lo[ax] + np.float32(k) * vsz[ax])
            for val in (edge, np.nextafter(edge, np.float32(-np.inf)), np.nextafter(edge, np.float32(np.inf))):
                p = np.array([r.uniform(rng_[0], rng_[3]), r.uniform(rng_[1], rng_[4]), r.uniform(rng_[2], rng_[5])],
                             np.float32)
                p[ax] = val
                rows.append(p)
    rows = np.asarray(rows, np.float32)
    # out-of-range on every side
    oor = np.array([[rng_[0] - 1, 0, 0], [rng_[3] + 5, 0, 0], [10, rng_[1] - 0.1, 0], [10, rng_[4] + 0.1, 0],
                    [10, 0, rng_[2] - 3], [10, 0, rng_[5] + 3], [rng_[3], rng_[4], rng_[5]], [rng_[0], rng_[1], rng_[2]]],
                   np.float32)
    p3 = np.concatenate([rows, oor], 0)
    rest = r.uniform(-1, 1, (p3.shape[0], 4)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([p3, rest], 1))


# ----------------------------------------------------------------------------- G1..G3
def gen_index():
    out = {}
    r = np.random.default_rng(11)
    cart = synth.synth_sweep_cart(400, seed=3)
    special = np.array([[0, 0, 0, .5, 0], [1, 0, 0, .5, 0], [-1, 0, 0, .5, 0], [-1, -0.0, 1, .1, 0], [0, 1, 0, .5, 0],
                        [0, -1, 0, .5, 0], [-2, 1e-7, 0, .5, 0], [-2, -1e-7, 0, .5, 0], [3, 4, -1, .2, .05],
                        [1e-3, 1e-3, 0, 0, 0], [49.9, 0.01, 2, 1, 0.45]], np.float32)
    cart = np.concatenate([special, cart], 0)
    out["cart_in"] = cart
    out["polar_out"] = transform_points(cart, "cylinder")
    assert out["polar_out"].dtype == np.float32
    for tag, rng_, vs in (("nusc", synth.NUSC_RANGE, synth.NUSC_VOXEL), ("coarse", synth.COARSE_RANGE, synth.COARSE_VOXEL),
                          ("waymo", synth.WAYMO_RANGE, synth.WAYMO_VOXEL)):
        vg = VoxelGenerator(list(vs), list(rng_), 5, 1000)
        grid = vg.grid_size
        pts = edge_points(rng_, vs, grid, seed=5)
        gi, shape, prange, vsize = ref_grid_ind(pts, rng_, vs)
        out[f"{tag}_grid_size"] = np.asarray(shape, np.int64)
        out[f"{tag}_range_f32"] = np.asarray(prange, np.float32)
        out[f"{tag}_voxel_f32"] = np.asarray(vsize, np.float32)
        out[f"{tag}_edge_pts"] = pts
        out[f"{tag}_edge_grid_ind"] = gi.astype(np.int32)
        # regenerable synthetic sweep
        n = 30000 if tag != "waymo" else 20000
        sw = synth.synth_sweep_polar(n, seed=0, rho_max=50.0 if tag != "waymo" else 74.0)
        gi2, *_ = ref_grid_ind(sw, rng_, vs)
        out[f"{tag}_sweep_n"] = np.int64(n)
        out[f"{tag}_sweep_grid_ind"] = gi2.astype(np.int32)
    # torch.unique triples (reference call: pillar_encoder.py:398) for B=1 and B=4
    gi_b1 = collate_grid_ind([out["nusc_sweep_grid_ind"].astype(np.int64)])
    u, inv, cnt = torch.unique(torch.from_numpy(gi_b1), return_inverse=True, return_counts=True, dim=0)
    out["nusc_b1_unq"] = u.numpy().astype(np.int32)
    out["nusc_b1_inv"] = inv.numpy().astype(np.int32)
    out["nusc_b1_cnt"] = cnt.numpy().astype(np.int32)
    gis = []
    for b in range(4):
        sw = synth.synth_sweep_polar(6000 + 500 * b, seed=100 + b, rho_max=20.0)
        g, *_ = ref_grid_ind(sw, synth.NUSC_RANGE, synth.NUSC_VOXEL)
        gis.append(g.astype(np.int64))
    gi_b4 = collate_grid_ind(gis)
    u, inv, cnt = torch.unique(torch.from_numpy(gi_b4), return_inverse=True, return_counts=True, dim=0)
    out["nusc_b4_grid_ind"] = gi_b4.astype(np.int32)
    out["nusc_b4_unq"] = u.numpy().astype(np.int32)
    out["nusc_b4_inv"] = inv.numpy().astype(np.int32)
    out["nusc_b4_cnt"] = cnt.numpy().astype(np.int32)
    # Waymo 3-D grid (Z=40) unique, edge points twice (duplicates) + sweep
    gw = collate_grid_ind([out["waymo_sweep_grid_ind"].astype(np.int64), out["waymo_edge_grid_ind"].astype(np.int64)])
    u, inv, cnt = torch.unique(torch.from_numpy(gw), return_inverse=True, return_counts=True, dim=0)
    out["waymo_b2_unq"] = u.numpy().astype(np.int32)
    out["waymo_b2_inv"] = inv.numpy().astype(np.int32)
    out["waymo_b2_cnt"] = cnt.numpy().astype(np.int32)
    save("index_cases.npz", **out)


# ----------------------------------------------------------------------------- G4
def gen_hard():
    out = {}
    # small 3-D polar grid, overflow of max_points and of max_voxels
    rng_ = (0.0, -1.0, -2.0, 8.0, 1.0, 2.0)
    vs = (0.5, 0.125, 1.0)  # 16 x 16 x 4
    r = np.random.default_rng(21)
    pts = np.stack([r.uniform(-0.5, 8.5, 3000), r.uniform(-1.1, 1.1, 3000), r.uniform(-2.2, 2.2, 3000)], 1)
    pts = np.concatenate([pts, r.uniform(-1, 1, (3000, 4))], 1).astype(np.float32)
    for tag, mp, mv in (("a", 5, 100000), ("b", 3, 300), ("c", 1, 50)):
        vg = VoxelGenerator(list(vs), list(rng_), mp, mv)
        voxels, coors, num, _, _ = vg.generate(pts)
        out[f"small_{tag}_max_points"] = np.int64(mp)
        out[f"small_{tag}_max_voxels"] = np.int64(mv)
        out[f"small_{tag}_voxels"] = voxels
        out[f"small_{tag}_coors"] = coors
        out[f"small_{tag}_num"] = num
    out["small_pts"] = pts
    out["small_range"] = np.asarray(rng_, np.float32)
    out["small_voxel"] = np.asarray(vs, np.float32)
    # Waymo grid, regenerable sweep, P=5, Vmax below the natural voxel count -> truncation
    sw = synth.synth_sweep_polar(20000, seed=0, rho_max=74.0)
    vg = VoxelGenerator(list(synth.WAYMO_VOXEL), list(synth.WAYMO_RANGE), 5, 15000)
    voxels, coors, num, _, _ = vg.generate(sw)
    out["waymo_n"] = np.int64(20000)
    out["waymo_max_voxels"] = np.int64(15000)
    out["waymo_coors"] = coors.astype(np.int16)
    out["waymo_num"] = num.astype(np.int8)
    out["waymo_voxels_sum"] = voxels.astype(np.float64).sum(axis=(1,)).astype(np.float32)[::16]
    # VoxelFeatureExtractorV3 (voxel_encoder.py:15-22) on the small case "a"
    vfe = VoxelFeatureExtractorV3(num_input_features=7)
    o = vfe(torch.from_numpy(out["small_a_voxels"]), torch.from_numpy(out["small_a_num"]))
    out["small_a_vfe"] = o.numpy()
    save("hard_voxel.npz", **out)


def clustered_sweep(n, seed, k=300):
    r = np.random.default_rng(seed)
    c_rho = r.uniform(2, 45, k)
    c_phi = r.uniform(-np.pi, np.pi, k)
    which = r.integers(0, k, n)
    rho = np.clip(c_rho[which] + 0.15 * r.standard_normal(n), 0.31, 50.4)
    phi = np.clip(c_phi[which] + 0.02 * r.standard_normal(n), -3.14, 3.14)
    z = r.uniform(-3, 1, n)
    cart = np.stack([rho * np.cos(phi), rho * np.sin(phi), z, r.uniform(0, 1, n), np.zeros(n)], 1).astype(np.float32)
    return np.ascontiguousarray(synth.cart_to_polar_host(cart))


def make_example(sweeps, rng_, vs):
    gis, shape = [], None
    for s in sweeps:
        g, shape, prange, vsize = ref_grid_ind(s, rng_, vs)
        gis.append(g.astype(np.int64))
    gi = collate_grid_ind(gis)
    ex = dict(points=torch.from_numpy(np.concatenate(sweeps, 0)), grid_ind=torch.from_numpy(gi),
              num_points=torch.tensor([len(s) for s in sweeps]), voxel_size=np.stack([vsize] * len(sweeps)),
              pc_range=np.stack([prange] * len(sweeps)), grid_size=np.stack([shape] * len(sweeps)))
    return ex


# ----------------------------------------------------------------------------- G5, G6, G7
def gen_reader():
    out = {}
    sweeps = [clustered_sweep(2500, 31), clustered_sweep(1800, 32)]
    ex = make_example(sweeps, synth.NUSC_RANGE, synth.NUSC_VOXEL)
    data = dict(points=ex["points"], grid_ind=ex["grid_ind"])
    out["points"] = ex["points"].numpy()
    out["grid_ind"] = ex["grid_ind"].numpy().astype(np.int32)
    enc = DynamicVoxelEncoderV1(num_input_features=7)
    f, unq = enc(data)
    out["dve_features"] = f.numpy()
    out["dve_unq"] = unq.numpy().astype(np.int32)
    pfn = DynamicPFNet(num_filters=[64, 128], num_input_features=7, voxel_shape="cylinder", xyz_cluster=True,
                       raz_cluster=True, xy_center=True, ra_center=True, voxel_size=list(synth.NUSC_VOXEL),
                       pc_range=list(synth.NUSC_RANGE)).eval()
    synth.load_filled(pfn, base_seed=1)
    with torch.no_grad():
        unq, unq_inv, _ = torch.unique(data["grid_ind"], return_inverse=True, return_counts=True, dim=0)
        deco = pfn.feature_deco(data["points"], unq_inv, data["grid_ind"])
        feats, unq2 = pfn(data)
        canvas = DynamicPPScatter()(feats, unq2, 2, [512, 512, 1])
    out["pfn_deco"] = deco.numpy()
    out["pfn_features"] = feats.numpy()
    out["pfn_unq"] = unq2.numpy().astype(np.int32)
    out["pfn_state_keys"] = np.array(list(pfn.state_dict().keys()))
    out["canvas_sum_c"] = canvas.double().sum(dim=(0, 2, 3)).numpy()  # per-channel checksum
    out["canvas_nnz"] = np.int64((canvas != 0).any(dim=1).sum())
    out["canvas_probe_idx"] = unq2.numpy()[::37].astype(np.int32)
    pidx = unq2[::37]
    out["canvas_probe_val"] = canvas[pidx[:, 0], :, pidx[:, 2], pidx[:, 3]].numpy()
    # cuboid variant of the decoration (voxel_shape='cuboid' branches, pillar_encoder.py:353-383)
    pfn2 = DynamicPFNet(num_filters=[32], num_input_features=7, voxel_shape="cuboid", xyz_cluster=True,
                        raz_cluster=False, xy_center=True, ra_center=False, voxel_size=[0.2, 0.2, 8],
                        pc_range=[-51.2, -51.2, -5, 51.2, 51.2, 3]).eval()
    synth.load_filled(pfn2, base_seed=2)
    with torch.no_grad():
        f2, u2 = pfn2(data)
    out["pfn_cuboid_features"] = f2.numpy()
    save("reader.npz", **out)


NUSC_TASKS = [dict(num_class=10, class_names=["car", "truck", "construction_vehicle", "bus", "trailer", "barrier",
                                              "motorcycle", "bicycle", "pedestrian", "traffic_cone"])]


def nusc_model_cfg(rng_, vs, pfn_filters=(64, 128), ds_filters=(128, 128, 256), us_filters=(128, 128, 128),
                   layer_nums=(3, 5, 5)):
    vg = dict(range=list(rng_), voxel_size=list(vs), max_points_in_voxel=20, max_voxel_num=[30000, 60000],
              voxel_shape="cylinder", return_density=True, dynamic=True, nsectors=1)
    head = dict(type="CenterHeadSinglePos", in_channels=sum(us_filters), tasks=NUSC_TASKS, dataset="nuscenes", weight=0.5,
                code_weights=[1.5, 1.5, 1.0, 1.0, 1.0, 1.0, 0.5, 0.5, 1.0, 1.0],
                common_heads={"reg": (2, 2), "rot_vel": (2, 2), "height": (1, 2), "dim": (3, 2)},
                voxel_shape="cylinder", voxel_generator=vg)
    return dict(type="PointPillars", pretrained=None,
                reader=dict(type="DynamicPFNet", num_filters=list(pfn_filters), num_input_features=7, voxel_shape="cylinder",
                            xyz_cluster=True, raz_cluster=True, xy_center=True, ra_center=True, voxel_size=list(vs),
                            pc_range=list(rng_)),
                backbone=dict(type="DynamicPPScatter", ds_factor=1),
                neck=dict(type="RPN", layer_nums=list(layer_nums), ds_layer_strides=[2, 2, 2], ds_num_filters=list(ds_filters),
                          us_layer_strides=[0.5, 1, 2], us_num_filters=list(us_filters), num_input_features=pfn_filters[-1],
                          logger=logging.getLogger("RPN")),
                bbox_head=head, seg_head=None, part_head=None)


def run_stages(model, ex, bs):
    """Run the reference forward stage by stage (point_pillars.py:40-53,55-110)."""
    data = dict(points=ex["points"], grid_ind=ex["grid_ind"], num_points=ex["num_points"], batch_size=bs,
                voxel_size=ex["voxel_size"][0], pc_range=ex["pc_range"][0], grid_size=ex["grid_size"][0])
    feats, unq = model.reader(data)
    x1 = model.backbone(feats, unq, bs, data["grid_size"])
    blocks, ups, x = [], [], x1
    for i in range(len(model.neck.blocks)):
        x = model.neck.blocks[i](x)
        blocks.append(x)
        if i - model.neck._upsample_start_idx >= 0:
            ups.append(model.neck.deblocks[i - model.neck._upsample_start_idx](x))
    x2 = torch.cat(ups, 1)
    preds = model.bbox_head(x2)
    return feats, unq, x1, blocks, ups, x2, preds


# ----------------------------------------------------------------------------- full C1/C2 model
def gen_full():
    out = {}
    cfg = nusc_model_cfg(synth.NUSC_RANGE, synth.NUSC_VOXEL)
    model = build_detector(cfg, train_cfg=None, test_cfg=None).eval()
    synth.load_filled(model, base_seed=0)
    out["state_keys"] = np.array(list(model.state_dict().keys()))
    out["state_shapes"] = np.array([str(tuple(v.shape)) for v in model.state_dict().values()])
    sw = synth.synth_sweep_polar(30000, seed=0)
    ex = make_example([sw], synth.NUSC_RANGE, synth.NUSC_VOXEL)
    with torch.no_grad():
        feats, unq, x1, blocks, ups, x2, preds = run_stages(model, ex, 1)
        whole = model(dict(ex, **{"num_points": ex["num_points"]}), return_loss=False) if False else None
    out["num_voxels"] = np.int64(feats.shape[0])
    out["pfn_features_head"] = feats[:512].numpy()
    out["pfn_features_sum_c"] = feats.double().sum(0).numpy()
    out["unq"] = unq.numpy().astype(np.int16)
    for i, b in enumerate(blocks):
        out[f"block{i}_s8"] = b[:, :, ::8, ::8].numpy()
        out[f"block{i}_sum_c"] = b.double().sum(dim=(0, 2, 3)).numpy()
    out["x2_s8"] = x2[:, :, ::8, ::8].numpy()
    out["x2_sum_c"] = x2.double().sum(dim=(0, 2, 3)).numpy()
    out["pos_encoding"] = model.bbox_head.pos_encoding.numpy()
    for k, v in preds["det_preds"][0].items():
        out[f"pred_{k}"] = v.numpy()
    save("full_c2.npz", **out)


# ----------------------------------------------------------------------------- small model, B=2, all stages + loss
SMALL_RANGE = synth.NUSC_RANGE
SMALL_VOXEL = (0.784, 0.0984, 8.0)  # 64 x 64 x 1 grid -> 16 x 16 BEV


def make_targets(bs, hw, seed, max_objs=500, n_pos=23):
    r = np.random.default_rng(seed)
    H, W = hw
    hm = (r.uniform(0, 1, (bs, 10, H, W)) ** 8).astype(np.float32)
    ind = np.zeros((bs, max_objs), np.int64)
    mask = np.zeros((bs, max_objs), np.uint8)
    cat = np.zeros((bs, max_objs), np.int64)
    anno = np.zeros((bs, max_objs, 10), np.float32)
    for b in range(bs):
        k = n_pos + 3 * b
        ind[b, :k] = r.choice(H * W, k, replace=False)
        mask[b, :k] = 1
        cat[b, :k] = r.integers(0, 10, k)
        anno[b, :k] = r.standard_normal((k, 10)).astype(np.float32)
        hm[b, cat[b, :k], ind[b, :k] // W, ind[b, :k] % W] = 1.0
    return hm, ind, mask, cat, anno


def gen_small():
    out = {}
    cfg = nusc_model_cfg(SMALL_RANGE, SMALL_VOXEL, pfn_filters=(32, 32), ds_filters=(32, 32, 64), us_filters=(32, 32, 32),
                         layer_nums=(1, 2, 2))
    model = build_detector(cfg, train_cfg=None, test_cfg=None).eval()
    synth.load_filled(model, base_seed=5)
    out["state_keys"] = np.array(list(model.state_dict().keys()))
    sweeps = [synth.synth_sweep_polar(3000, seed=41), clustered_sweep(2000, 42, k=60)]
    ex = make_example(sweeps, SMALL_RANGE, SMALL_VOXEL)
    out["points"] = ex["points"].numpy()
    out["grid_ind"] = ex["grid_ind"].numpy().astype(np.int32)
    with torch.no_grad():
        feats, unq, x1, blocks, ups, x2, preds = run_stages(model, ex, 2)
    out["pfn_features"] = feats.numpy()
    out["unq"] = unq.numpy().astype(np.int32)
    out["canvas"] = x1.numpy()
    for i, b in enumerate(blocks):
        out[f"block{i}"] = b.numpy()
    for i, u in enumerate(ups):
        out[f"up{i}"] = u.numpy()
    for k, v in preds["det_preds"][0].items():
        out[f"pred_{k}"] = v.numpy()
    # head internals (center_head_parallel.py:262-284)
    with torch.no_grad():
        h = model.bbox_head
        xs = h.shared_conv(x2)
        out["head_shared"] = xs.numpy()
        out["head_cal_weight"] = h.calibration_weight(h.pos_encoding).numpy()
        out["head_cal_bias"] = h.calibration_bias(h.pos_encoding).numpy()
        out["pos_encoding"] = h.pos_encoding.numpy()
    # loss (center_head.py:248-288) in eval mode on the eval predictions
    hm, ind, mask, cat, anno = make_targets(2, (16, 16), seed=77)
    example = dict(hm=[torch.from_numpy(hm)], ind=[torch.from_numpy(ind)], mask=[torch.from_numpy(mask)],
                   cat=[torch.from_numpy(cat)], anno_box=[torch.from_numpy(anno)])
    out["tgt_hm"], out["tgt_ind"], out["tgt_mask"], out["tgt_cat"], out["tgt_anno"] = hm, ind, mask, cat, anno
    with torch.no_grad():
        _, _, _, _, _, _, preds2 = run_stages(model, ex, 2)
        losses = model.bbox_head.loss(example, preds2)
    out["loss_det"] = np.float64(losses["det_loss"][0])
    out["loss_hm"] = np.float64(losses["hm_loss"][0])
    out["loss_loc_elem"] = losses["loc_loss_elem"][0].numpy()
    # train-mode step: forward (batch-stat BN), loss, backward -> a few grads
    model.train()
    synth.load_filled(model, base_seed=5)
    _, _, _, tblocks, _, tx2, tpreds = run_stages(model, ex, 2)
    tl = model.bbox_head.loss(example, tpreds)
    loss = sum(tl["det_loss"])
    loss.backward()
    out["train_loss_det"] = np.float64(loss.detach())
    out["train_block0"] = tblocks[0].detach().numpy()
    named = dict(model.named_parameters())
    for pn in ("reader.pfn_layers.0.linear.weight", "reader.pfn_layers.1.linear.weight", "neck.blocks.0.1.weight",
               "neck.blocks.2.4.weight", "neck.deblocks.2.0.weight", "bbox_head.shared_conv.0.weight",
               "bbox_head.hm.3.weight", "bbox_head.reg.0.conv.0.weight", "bbox_head.calibration_weight.0.weight"):
        out["grad::" + pn] = named[pn].grad.numpy()
    out["train_bn_running_mean"] = model.neck.blocks[0][2].running_mean.numpy()
    out["train_bn_running_var"] = model.neck.blocks[0][2].running_var.numpy()
    save("small_model.npz", **out)


# ----------------------------------------------------------------------------- H1 plain CenterHead + CenterHeadSingle
def gen_heads():
    out = {}
    tasks = [dict(num_class=2, class_names=["a", "b"]), dict(num_class=1, class_names=["c"])]
    h = CenterHead(in_channels=24, tasks=tasks, dataset="nuscenes", weight=0.25, code_weights=[1.0] * 10,
                   common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}).eval()
    synth.load_filled(h, base_seed=8)
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((2, 24, 12, 20)).astype(np.float32))
    with torch.no_grad():
        p = h(x.clone())
    out["ch_x"] = x.numpy()
    out["ch_state_keys"] = np.array(list(h.state_dict().keys()))
    for t, d in enumerate(p["det_preds"]):
        for k, v in d.items():
            out[f"ch_t{t}_{k}"] = v.numpy()
    hs = CenterHeadSingle(in_channels=24, tasks=NUSC_TASKS, dataset="nuscenes", weight=0.25, code_weights=[1.0] * 10,
                          common_heads={"reg": (2, 2), "rot_vel": (2, 2), "height": (1, 2), "dim": (3, 2)},
                          voxel_shape="cylinder").eval()
    synth.load_filled(hs, base_seed=10)
    x = torch.from_numpy(np.random.default_rng(12).standard_normal((2, 24, 12, 32)).astype(np.float32))
    with torch.no_grad():
        p = hs(x.clone())
    out["chs_x"] = x.numpy()
    out["chs_state_keys"] = np.array(list(hs.state_dict().keys()))
    for k, v in p["det_preds"][0].items():
        out[f"chs_{k}"] = v.numpy()
    save("heads.npz", **out)


# ----------------------------------------------------------------------------- A1 SetBlock (reduced + full-size probe)
def bev_pos(H, W, vs, rng_, scale):
    """Cartesian/polar cell-centre positions, same construction as voxelnet.py:10-25 for (H=r, W=theta)."""
    by, bx = torch.meshgrid(torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W))
    bx, by = bx + 0.5, by + 0.5
    r = by * vs[0] * scale + rng_[0]
    phi = bx * vs[1] * scale + rng_[1]
    return torch.stack([r * torch.cos(phi), r * torch.sin(phi), r, phi], dim=2)[None]


def gen_setblock():
    out = {}
    H, W, C = 16, 32, 64
    pos = bev_pos(H, W, (0.065 * 9, 0.00307 * 8, 0.15), synth.WAYMO_RANGE, 8)
    out["pos"] = pos.numpy()
    x = torch.from_numpy(np.random.default_rng(51).standard_normal((2, H * W, C)).astype(np.float32))
    out["x"] = x.numpy()
    for shift in (False, True):
        blk = SetBlock(in_dim=C, embed_dim_scale=1, num_heads=4, reso=(H, W), mlp_ratio=4., qkv_bias=True, qk_scale=None,
                       H_sp=H, W_sp=1, H=4, W=8, drop=0.1, attn_drop=0.1, drop_path=0.1, norm_layer=torch.nn.LayerNorm,
                       pos=pos, shift=shift).eval()
        synth.load_filled(blk, base_seed=60 + int(shift))
        # the key-point rows the reference picked: SectorAttention receives the gathered key-point positions (s_pos) next to the
        # full position map (x_pos, rolled for the shifted block); every BEV cell has its own position, so matching them back gives
        # the reference's top_idx, including its resolution of the ties among zero scores (unstable argsort, set_transformer.py:143)
        seen = {}
        hook = blk.attns.sector_attn1.register_forward_pre_hook(lambda mod, args: seen.update(s_pos=args[2].clone(), x_pos=args[3].clone()))
        with torch.no_grad():
            y = blk(x)
            xn = blk.attns.norm1(x).view(2, H, W, C)
        hook.remove()
        tag = "shift" if shift else "noshift"
        out[f"y_{tag}"] = y.numpy()
        s_pos, x_pos = seen["s_pos"], seen["x_pos"].expand(2, -1, -1, -1)                 # (B, K, W, 2), (B, H, W, 2)
        match = (s_pos[:, :, None, :, :] == x_pos[:, None, :, :, :]).all(-1)             # (B, K, H, W)
        assert bool((match.sum(2) == 1).all())
        out[f"top_{tag}"] = match.float().argmax(2).numpy().astype(np.int16)             # (B, K, W) rows in the (rolled) frame
        # how tie-heavy the case is: columns with fewer than K positive strict-interior local maxima have to fill up from the zeros
        if shift:
            xn = torch.roll(xn, -4, 2)
        sc = xn.mean(3)                                                                   # (B, H, W)
        inner = sc[:, 1:-1]
        lm = (inner >= sc[:, :-2]) & (inner >= sc[:, 2:]) & (inner > 0)
        out[f"tie_cols_{tag}"] = np.array(int((lm.sum(1) < 4).sum()))
        out[f"state_keys_{tag}"] = np.array(list(blk.state_dict().keys()))
    save("setblock_small.npz", **out)
    # full-size Waymo-shape block pair (voxelnet.py:192-199): probes + checksums only
    import det3d.models.detectors.voxelnet as vn
    H, W, C = 144, 256, 256
    x = torch.from_numpy(np.random.default_rng(52).standard_normal((1, H * W, C)).astype(np.float32))
    o = {}
    y = x
    for i in range(2):
        blk = SetBlock(in_dim=256, embed_dim_scale=1, num_heads=4, reso=(144, 256), mlp_ratio=4., qkv_bias=True,
                       qk_scale=None, H_sp=144, W_sp=1, H=4, W=8, drop=0.1, attn_drop=0.1, drop_path=0.1,
                       norm_layer=torch.nn.LayerNorm, pos=vn.bev_pos, shift=(i % 2 == 1)).eval()
        synth.load_filled(blk, base_seed=70 + i)
        with torch.no_grad():
            y = blk(y)
        o[f"y{i}_probe"] = y[0, ::97, :].numpy()
        o[f"y{i}_sum_c"] = y.double().sum(dim=(0, 1)).numpy()
    # the shifted block again on an input of its own (key-point selection is discontinuous: the chained
    # result above is sensitive to 1e-6 differences in the first block's output)
    x2 = torch.from_numpy(np.random.default_rng(53).standard_normal((1, H * W, C)).astype(np.float32))
    with torch.no_grad():
        y2 = blk(x2)  # blk is the shift=True block with seed 71
    o["y1_indep_probe"] = y2[0, ::97, :].numpy()
    o["y1_indep_sum_c"] = y2.double().sum(dim=(0, 1)).numpy()
    o["bev_pos_probe"] = vn.bev_pos[0, ::13, ::17, :].numpy()
    save("setblock_full.npz", **o)


# ----------------------------------------------------------------------------- T1 optimizer step
def gen_optim():
    """Reference OptimWrapper (decoupled wd, Adam betas=(mom,0.99)) + OneCycle + clip_grad_norm_(35)
    on a toy module: conv + BatchNorm + conv, 7 steps of a 50-step schedule with seeded grads.
    Stores lr/mom per step, the total gradient norm and the parameters after each step."""
    from functools import partial
    from torch import nn
    from torch.nn.utils import clip_grad
    from det3d.solver.fastai_optim import OptimWrapper
    from det3d.solver.learning_schedules_fastai import OneCycle
    from det3d.torchie.apis.train import flatten_model
    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv2d(4, 6, 3, bias=False), nn.BatchNorm2d(6), nn.ReLU(), nn.Conv2d(6, 3, 1, bias=True))
    rng = np.random.default_rng(42)
    names = [n for n, _ in model.named_parameters()]
    for n, p_ in model.named_parameters():
        p_.data = torch.from_numpy(rng.standard_normal(tuple(p_.shape)).astype(np.float32) * 0.3)
    opt = OptimWrapper.create(partial(torch.optim.Adam, betas=(0.9, 0.99), amsgrad=0.0), 3e-3, [nn.Sequential(*flatten_model(model))],
                              wd=0.01, true_wd=True, bn_wd=True)
    total_step = 50
    sched = OneCycle(opt, total_step, 0.005, [0.95, 0.85], 10.0, 0.4)
    out = {"names": np.array(names), "total_step": total_step}
    for n, p_ in model.named_parameters():
        out["init::" + n] = p_.detach().numpy().copy()
    lrs, moms, norms = [], [], []
    steps = (0, 1, 2, 19, 20, 21, 49)   # crosses the pct_start boundary (a1 = 20)
    for step in steps:
        sched.step(step)
        lrs.append(opt.lr); moms.append(opt.mom)
        for n, p_ in model.named_parameters():
            scale = 40.0 if step in (1, 20) else 1.0   # clip (max_norm 35) active on these steps
            p_.grad = torch.from_numpy(rng.standard_normal(tuple(p_.shape)).astype(np.float32) * scale)
            out[f"grad{step}::" + n] = p_.grad.numpy().copy()
        tn = clip_grad.clip_grad_norm_(filter(lambda q: q.requires_grad, model.parameters()), max_norm=35, norm_type=2)
        norms.append(float(tn))
        opt.step()
        for n, p_ in model.named_parameters():
            out[f"after{step}::" + n] = p_.detach().numpy().copy()
    out["steps"] = np.array(steps)
    out["lr"], out["mom"], out["total_norm"] = np.array(lrs, np.float64), np.array(moms, np.float64), np.array(norms, np.float64)
    save("optim.npz", **out)


# ----------------------------------------------------------------------------- next-3 target assignment
def gen_assign():
    """AssignLabel.assign_heatmap_polar (preprocess.py:253-342) on seeded boxes: hm / ind / mask / cat / anno_box, with the
    dtypes the pipeline hands it (float32 voxel_size / pc_range arrays from VoxelGenerator)."""
    import types
    from det3d.datasets.pipelines.preprocess import AssignLabel
    out = {}
    vs, pr = np.array(synth.NUSC_VOXEL, np.float32), np.array(synth.NUSC_RANGE, np.float32)
    fmap = np.array([512, 512, 1]) [:2] // 4
    for tag, n, rectify, seed in (("a", 60, False, 1), ("b", 140, True, 2)):
        boxes, classes = synth.synth_gt_boxes(n, seed)
        me = types.SimpleNamespace(_max_objs=100, out_size_factor=4, gaussian_overlap=0.1, _min_radius=2, rectify=rectify)
        hms = [np.zeros((10, fmap[1], fmap[0]), np.float32)]
        inds, masks, cats = [np.zeros(100, np.int64)], [np.zeros(100, np.uint8)], [np.zeros(100, np.int64)]
        annos = [np.zeros((100, 10), np.float32)]
        AssignLabel.assign_heatmap_polar(me, hms, annos, inds, masks, cats, dict(gt_boxes=[boxes.copy()], gt_classes=[classes.copy()]),
                                         [None], vs, pr, fmap, "NuScenesDataset")
        out[f"{tag}_n"], out[f"{tag}_rectify"], out[f"{tag}_seed"] = n, rectify, seed
        nz = np.nonzero(hms[0])
        out[f"{tag}_hm_idx"] = np.stack(nz, 1).astype(np.int32)
        out[f"{tag}_hm_val"] = hms[0][nz]
        out[f"{tag}_ind"], out[f"{tag}_mask"], out[f"{tag}_cat"], out[f"{tag}_anno"] = inds[0], masks[0], cats[0], annos[0]
    save("assign.npz", **out)


# ----------------------------------------------------------------------------- next-4 sweep accumulation
def gen_sweeps():
    """read_sweep (loading.py:73-84) + the key-frame concatenation of LoadPointCloudFromFile.get_points (:216-250) on temp .bin
    files: 1 key frame + 3 past sweeps with rigid transforms and time lags; stores the accumulated (N', 5) cloud."""
    import tempfile
    from det3d.datasets.pipelines.loading import read_file, read_sweep
    clouds, mats, lags = synth.synth_raw_sweeps(4, 2500, seed=5)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, c in enumerate(clouds):
            paths.append(os.path.join(d, f"s{i}.bin"))
            c.astype(np.float32).tofile(paths[-1])
        points = read_file(paths[0])
        pts_list, t_list = [points], [np.zeros((points.shape[0], 1))]
        for i in range(1, 4):
            ps, ts = read_sweep(dict(lidar_path=paths[i], transform_matrix=mats[i], time_lag=float(lags[i])))
            pts_list.append(ps); t_list.append(ts)
        pts = np.concatenate(pts_list, 0)
        times = np.concatenate(t_list, 0).astype(pts.dtype)
        acc = np.hstack([pts, times])
    save("sweeps.npz", accumulated=acc.astype(np.float32), counts=np.array([len(p) for p in pts_list]))


# ----------------------------------------------------------------------------- V4 static twin: PillarFeatureNet
def gen_pillar_static():
    """PillarFeatureNet.forward (pillar_encoder.py:131-169) + PFNLayer.forward_static (:47-60), eval mode, on hard voxels of a
    synthetic Cartesian sweep: one layer (64,) and two layers (64, 128) with the distance feature."""
    from det3d.models.readers.pillar_encoder import PillarFeatureNet
    pts = synth.synth_sweep_cart(6000, seed=3)[:, :4].copy()
    rng_, vs = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], [0.8, 0.8, 8.0]
    vg = VoxelGenerator(vs, rng_, 20, 1500)
    voxels, coors, num = vg.generate(pts, 1500)[:3]
    coors4 = np.concatenate([np.zeros((len(coors), 1), coors.dtype), coors], 1)
    out = dict(voxels=voxels.astype(np.float32), coors=coors4.astype(np.int32), num=num.astype(np.int32))
    for tag, filters, dist in (("one", (64,), False), ("two", (64, 128), True)):
        net = PillarFeatureNet(num_input_features=4, num_filters=filters, with_distance=dist, voxel_size=vs, pc_range=rng_).eval()
        synth.load_filled(net, base_seed=41)
        with torch.no_grad():
            y = net(torch.from_numpy(out["voxels"]), torch.from_numpy(out["num"]), torch.from_numpy(coors4.astype(np.int64)))
        out[f"{tag}_features"] = y.numpy()
        out[f"{tag}_keys"] = np.array(list(net.state_dict().keys()))
    save("pillar_static.npz", **out)


# ----------------------------------------------------------------------------- segmentation head (the config's `seg` super-task)
def gen_seg_head():
    """SingleConvHead of the reference (seg_heads/seg_head.py:53-83, 176-195) on a small canvas + RPN map, eval: logits and the
    per-point labels of its predict()"""
    from det3d.models.seg_heads.seg_head import SingleConvHead
    head = SingleConvHead(kernel=1, num_classes=6, in_channels=8 + 12, weight=2, loss=dict(type="SegLoss", ignore=-1)).eval()
    synth.load_filled(head, base_seed=77)
    r = np.random.default_rng(3)
    x1 = torch.from_numpy(r.standard_normal((2, 8, 16, 24)).astype(np.float32))
    x2 = torch.from_numpy(r.standard_normal((2, 12, 4, 6)).astype(np.float32))
    with torch.no_grad():
        preds = head(x1, x2)
    gi = [np.stack([np.zeros(50, np.int64), r.integers(0, 16, 50), r.integers(0, 24, 50)], 1) for _ in range(2)]
    example = dict(num_points=[50, 50], metadata=[dict(token="a"), dict(token="b")], valid_grid_ind=[torch.from_numpy(g) for g in gi])
    labels = [list(d.values())[0].numpy() for d in head.predict(example, preds, None)]
    save("seg_head.npz", x1=x1.numpy(), x2=x2.numpy(), seg_preds=preds["seg_preds"].numpy(), gi0=gi[0], gi1=gi[1], labels0=labels[0],
         labels1=labels[1], state_keys=np.array(list(head.state_dict().keys())))


WAYMO_HEAD_GT = dict(max_volumn_space=[75.18, 3.14368, 4.0], min_volumn_space=[0.3, -3.14368, -2.0], grid_size=[1152, 2048, 40])


def gen_e2e():
    """training side of the geometry-aware head: GroundTruthProcessor (vote map), CenterCoder, TimeMatcher and -- with the names
    loss_utils.py:7 fails to import injected as placeholders -- SetCriterion, all run from the reference on synthetic Waymo-size
    inputs (B = 2, 256 x 144 map).  The IoU term needs a CUDA-only extension and is not captured."""
    import importlib
    from det3d.models.bbox_heads.e2e_modules import GroundTruthProcessor
    from det3d.models.e2e_utils.box_coder_utils import CenterCoder
    from det3d.models.e2e_utils.matcher import TimeMatcher
    import det3d.core.utils.center_utils as cu
    for nm in ("bbox3d_overlaps_iou", "bbox3d_overlaps_giou", "bbox3d_overlaps_diou"):   # names loss_utils.py:7 expects (unused by the config's losses)
        if not hasattr(cu, nm):
            setattr(cu, nm, None)
    set_crit = importlib.import_module("det3d.models.e2e_utils.set_crit")
    from oracle import polar_oracle as O
    tasks = [ADict(num_class=1, class_names=["Vehicle"])]
    cfg = ADict(tasks=tasks, generate_votemap=True, feature_map_stride=8, gaussian_overlap=0.1, min_radius=4, num_max_objs=500, scale_factor=2,
                mapping={"Vehicle": 1}, **WAYMO_HEAD_GT)
    gtp = GroundTruthProcessor(gt_processor_cfg=cfg)
    B, H, W = 2, 256, 144
    gbox = synth.synth_vehicle_boxes(B, 48, seed=5)
    gt = gtp.process(torch.from_numpy(gbox))[0]
    vm = gt["votemap"].numpy()
    nz = np.argwhere(np.abs(vm).sum(-1) != 0)
    out = dict(global_box_seed=np.int64(5), vm_idx=nz.astype(np.int32), vm_val=vm[nz[:, 0], nz[:, 1], nz[:, 2]], vm_shape=np.array(vm.shape),
               gt_counts=np.array([len(x) for x in gt["gt_classes"]]))
    for b in range(B):
        out[f"gt_boxes{b}"] = gt["gt_boxes"][b].numpy()
    coder = CenterCoder(code_size=7, encode_angle_by_sincos=True, period=2 * np.pi)
    og = O.swv_offset_grid(WAYMO_HEAD_GT["grid_size"], 8, WAYMO_HEAD_GT["min_volumn_space"], WAYMO_HEAD_GT["max_volumn_space"])
    preds = {k: torch.from_numpy(v) for k, v in synth.synth_swv_preds(B, H, W, seed=9, boxes=gbox, offset_grid=og[0].numpy()).items()}
    anno = torch.cat([preds["reg"], preds["height"], preds["dim"], preds["rot"]], 1)
    pb = torch.cat([anno[:, :2] + og, anno[:, 2:]], 1).permute(0, 2, 3, 1).reshape(B, H * W, 8)
    pc = (preds["pred_centers"] + og).permute(0, 2, 3, 1).reshape(B, H * W, 2)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, -1)  # noqa: E731
    out["enc0"] = coder.encode(gt["gt_boxes"])[0].numpy()
    n0 = len(gt["gt_boxes"][0])
    out["delta0"] = coder.get_delta(gt_boxes=gt["gt_boxes"][0], preds=pb[0, :n0]).numpy()
    out["dec0"] = coder.decode_torch(pb[0, :64]).numpy()
    mcfg = dict(weight_dict={"loss_ce": 0.25, "loss_bbox": 0.75}, losses=["loss_ce", "loss_bbox"], code_weights=[1.0] * 8, use_focal_loss=True,
                box_pred_metric="loss_bbox", use_heatmap=False, box_coder=coder, period=2 * np.pi)
    matcher = TimeMatcher(**mcfg)
    pd = dict(pred_logits=flat(preds["hm"]), pred_boxes=pb, pred_centers=pc, pred_vote_cls=flat(preds["pred_vote_cls"]))
    inds = matcher(pd, gt)["inds"]
    for b in range(B):
        out[f"match_src{b}"], out[f"match_tgt{b}"] = inds[b][0].numpy(), inds[b][1].numpy()
    crit = set_crit.SetCriterion(matcher=matcher, weight_dict={"loss_ce": 1, "loss_bbox": 2, "loss_vote": 0.25, "loss_vote_cls": 1, "loss_iou": 2},
                                 losses=["loss_ce", "loss_bbox", "loss_vote", "loss_vote_cls"], sigma=3.0, box_coder=coder, code_weights=[1.0] * 8,
                                 gamma=2.0, alpha=0.25, use_focal_loss=True)
    for k in pd:
        pd[k] = pd[k].clone().requires_grad_(True)
    ls = crit(pd, gt)
    for k in ("loss_ce", "loss_bbox", "loss_vote", "loss_vote_cls", "loc_loss_elem", "loss"):
        out["crit_" + k] = ls[k].detach().numpy()
    ls["loss"].backward()
    # gradients of the four pinned terms w.r.t. the predictions (sparse where they are sparse)
    out["g_logits_sum"] = np.array([float(pd["pred_logits"].grad.double().sum()), float(pd["pred_logits"].grad.double().abs().sum())])
    gb = pd["pred_boxes"].grad
    gnz = np.argwhere(gb.abs().sum(-1).numpy() != 0)
    out["g_boxes_idx"], out["g_boxes_val"] = gnz.astype(np.int32), gb.numpy()[gnz[:, 0], gnz[:, 1]]
    gc = pd["pred_centers"].grad
    cnz = np.argwhere(gc.abs().sum(-1).numpy() != 0)
    out["g_centers_idx"], out["g_centers_val"] = cnz.astype(np.int32), gc.numpy()[cnz[:, 0], cnz[:, 1]]
    out["g_vote_cls_sum"] = np.array([float(pd["pred_vote_cls"].grad.double().sum()), float(pd["pred_vote_cls"].grad.double().abs().sum())])
    out["g_logits_at_matches"] = np.concatenate([pd["pred_logits"].grad[b, inds[b][0], 0].numpy() for b in range(B)])
    save("e2e_loss.npz", **out)


STREAM_NECK = dict(layer_nums=[1, 2], ds_layer_strides=[2, 2], ds_num_filters=[16, 32], us_layer_strides=[1, 2], us_num_filters=[16, 16],
                   num_input_features=8)


def gen_stream():
    """sector streaming: the reference's Voxelization.voxelize_streaming_polar on a 4-sector split of a synthetic sweep, and its
    context-padding necks RPNTECP (two chained sectors) and RPNBDCP (feature_only with 1 and 4 stacked sectors; streaming mode
    with a previous sweep for the first / a middle / the last sector) on small maps"""
    from det3d.models.necks.rpn_context import RPNTECP, RPNBDCP
    out = {}
    # ---- streaming voxelization
    cfg = ADict(vox_cfg(synth.NUSC_RANGE, synth.NUSC_VOXEL), nsectors=4)
    vx = Voxelization(cfg=cfg, super_tasks=["det"])
    pts = synth.synth_sweep_polar(6000, seed=77, rho_max=55.0)
    res = {"mode": "val", "lidar": {"points": pts.copy()}}
    secs, _ = vx.voxelize_streaming_polar(res, {})
    for i, sec in enumerate(secs["sectors"]):
        out[f"sec{i}_points"] = sec["lidar"]["points"].astype(np.float32)
        out[f"sec{i}_grid_ind"] = np.ascontiguousarray(sec["lidar"]["voxels"]["grid_ind"]).astype(np.int32)
    out["sec_shape"] = np.asarray(secs["sectors"][0]["lidar"]["voxels"]["shape"])
    # ---- necks
    logger = logging.getLogger("RPN")
    rng = np.random.default_rng(3)
    for name, cls, kw in (("tecp", RPNTECP, {}), ("bdcp", RPNBDCP, dict(nsectors=4))):
        torch.manual_seed(0)
        neck = cls(logger=logger, **STREAM_NECK, **kw).eval()
        sd = synth.fill_state_dict(neck.state_dict(), 21)
        neck.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        out[f"{name}_state_keys"] = np.array(list(neck.state_dict().keys()))
        xs = [torch.from_numpy(rng.standard_normal((2, 8, 16, 24)).astype(np.float32)) for _ in range(4)]
        with torch.no_grad():
            if name == "tecp":
                y0, ctx = neck(xs[0])
                y1, ctx1 = neck(xs[1], prev_context=[c.clone() for c in ctx], sec_id=1)
                out["tecp_y0"], out["tecp_y1"] = y0.numpy(), y1.numpy()
                out["tecp_ctx_shapes"] = np.array([list(c.shape) for c in ctx])
                out["tecp_ctx1_last"] = ctx1[-1].numpy()
            else:
                full = torch.cat(xs, 2)                                     # a full sweep: 64 azimuth rows
                y, cur_full = neck(full, nsectors=1, mode="feature_only")
                out["bdcp_full"] = y.numpy()
                stacked = torch.cat(xs, 0)                                  # 4 sectors x batch 2, sector-major
                ys, _ = neck(stacked, nsectors=4, mode="feature_only")
                out["bdcp_stacked"] = ys.numpy()
                # streaming over the sectors of a NEW sweep with the previous sweep's per-layer inputs as leading-edge context
                xn = [torch.from_numpy(rng.standard_normal((2, 8, 16, 24)).astype(np.float32)) for _ in range(4)]
                prev_ctx = []
                for sec in range(4):
                    yy, cur = neck(xn[sec], prev_sweep=cur_full, prev_context=[c for c in prev_ctx], sec_id=sec, nsectors=4, mode="eval")
                    out[f"bdcp_stream{sec}"] = yy.numpy()
                    prev_ctx = cur
    save("stream.npz", **out)


# ----------------------------------------------------------------------------- next-4 PolarStreamBDCP (two sweeps, ego-rotation warp)
BDCP_VOXEL = (0.784, 0.0984 / 2, 8.0)
BDCP_ANGLES = (0.04, -0.06)


def gen_stream_bdcp():
    """the reference's PolarStreamBDCP on CPU (torch.cuda.current_device patched to name the CPU for its mesh grids): two synthetic
    sweeps of batch 2 split into 4 sectors by the reference's own voxelize_streaming_polar + collate; stored: the warped per-layer
    maps of the previous sweep (what forward_one_sweep('feature_only') returns) and the raw head tensors of the current sweep
    (a forward hook on the head; the hook ends the call before the reference's CUDA NMS)"""
    nsec, batch = 4, 2
    rng_ = list(synth.NUSC_RANGE)
    heads = {"reg": (2, 2), "rot_vel": (2, 2), "height": (1, 2), "dim": (3, 2)}
    cfg = dict(type="PolarStreamBDCP", nsectors=nsec, pretrained=None,
               reader=dict(type="DynamicPFNet", num_filters=[32, 32], num_input_features=7, voxel_shape="cylinder", xyz_cluster=True, raz_cluster=True,
                           xy_center=True, ra_center=True, voxel_size=list(BDCP_VOXEL), pc_range=rng_),
               backbone=dict(type="DynamicPPScatter", ds_factor=1),
               neck=dict(type="RPNBDCP", layer_nums=[1, 1], ds_layer_strides=[2, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2], us_num_filters=[32, 32],
                         num_input_features=32, logger=logging.getLogger("RPN")),
               bbox_head=dict(type="CenterHeadSingle", in_channels=64, tasks=NUSC_TASKS, dataset="nuscenes", weight=0.5, code_weights=[1.0] * 10,
                              common_heads=heads, voxel_shape="cylinder"),
               seg_head=None, part_head=None)
    test_cfg = ADict(pc_range=rng_, stateful_nms=True)
    model = build_detector(cfg, train_cfg=None, test_cfg=test_cfg).eval()
    synth.load_filled(model, base_seed=23)
    vx = Voxelization(cfg=ADict(vox_cfg(synth.NUSC_RANGE, BDCP_VOXEL), nsectors=nsec), super_tasks=["det"])
    tm = np.stack([np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], np.float32) for a in BDCP_ANGLES])

    def example(seed):
        per_sample = []
        for b in range(batch):
            pts = synth.synth_sweep_polar(2500 + 100 * b, seed=seed + b)
            secs, _ = vx.voxelize_streaming_polar({"mode": "val", "lidar": {"points": pts.copy()}}, {})
            per_sample.append(secs["sectors"])
        pts, gis, num = [], [], []
        for sec in range(nsec):
            for b in range(batch):
                sd = per_sample[b][sec]["lidar"]
                gi = np.ascontiguousarray(sd["voxels"]["grid_ind"]).astype(np.int64)
                pts.append(sd["points"].astype(np.float32))
                gis.append(np.pad(gi, ((0, 0), (1, 0)), constant_values=sec * batch + b))
                num.append(len(gi))
        shape = np.asarray(per_sample[0][0]["lidar"]["voxels"]["shape"])
        n = nsec * batch
        return dict(points=torch.from_numpy(np.concatenate(pts)), grid_ind=torch.from_numpy(np.concatenate(gis)), num_points=torch.tensor(num),
                    voxel_size=np.stack([np.asarray(BDCP_VOXEL)] * n), pc_range=np.stack([np.asarray(rng_)] * n), grid_size=np.stack([shape] * n),
                    metadata=[None] * n, transform_matrix=torch.from_numpy(np.concatenate([tm] * nsec)))

    class _Done(Exception):
        pass
    grabbed = {}

    def hook(mod, inp, outp):
        grabbed["preds"] = outp
        raise _Done
    out = {"angles": np.asarray(BDCP_ANGLES)}
    real = torch.cuda.current_device
    torch.cuda.current_device = lambda: "cpu"
    try:
        with torch.no_grad():
            prev = model.forward_one_sweep(example(70), "feature_only", False)
            h = model.bbox_head.register_forward_hook(hook)
            try:
                model.forward_one_sweep(example(80), "eval", False, prev_sweep=prev)
            except _Done:
                pass
            h.remove()
    finally:
        torch.cuda.current_device = real
    for i, p in enumerate(prev):
        out[f"warped{i}"] = p.numpy() if i == len(prev) - 1 else p[:, ::4].numpy()      # every fourth channel of the larger maps
    for k, v in grabbed["preds"]["det_preds"][0].items():
        out[f"pred_{k}"] = v.numpy()
    save("stream_bdcp.npz", **out)


# ----------------------------------------------------------------------------- next-4 global augmentation
def gen_augment():
    """the reference's own augmentation functions under seeded np.random: inputs, outputs, and the seeds (the host side of the
    port re-draws from the same seed in the same order)"""
    from det3d.core.sampler import preprocess as prep
    out = {}
    rng = np.random.default_rng(7)
    for case, (cols, std) in enumerate(((9, 0.0), (7, [0.5, 0.5, 0.2]), (9, 0.3), (7, 0.0))):
        pts = (rng.standard_normal((1200, 5)) * np.array([20, 20, 2, 1, 0.1])).astype(np.float32)
        boxes = rng.standard_normal((37, cols)).astype(np.float32)
        boxes[:, :2] *= 25
        boxes[:, 3:6] = np.abs(boxes[:, 3:6]) + 0.5
        out[f"pts_{case}"], out[f"boxes_{case}"] = pts.copy(), boxes.copy()
        seed = 100 + case
        np.random.seed(seed)
        b, p = prep.random_flip_both(boxes.copy(), pts.copy())
        b, p = prep.global_rotation(b, p, rotation=[-0.78539816, 0.78539816])
        b, p = prep.global_scaling_v2(b, p, 0.95, 1.05)
        b, p = prep.global_translate_(b, p, noise_translate_std=std)
        out[f"pts_out_{case}"], out[f"boxes_out_{case}"] = p, b
        out[f"seed_{case}"] = np.array(seed)
        out[f"std_{case}"] = np.asarray(std, np.float64).reshape(-1)
    save("augment.npz", **out)


# ----------------------------------------------------------------------------- next-2 double-flip test-time augmentation
def gen_double_flip():
    """CenterHead.double_flip_decode of the reference on random head maps (two groups of four flipped copies)"""
    from det3d.models.bbox_heads.center_head import CenterHead
    rng = np.random.default_rng(17)
    shapes = dict(hm=3, reg=2, height=1, dim=3, rot=2, vel=2)
    inp = {k: rng.standard_normal((8, 6, 5, c)).astype(np.float32) for k, c in shapes.items()}
    out = {f"in_{k}": v for k, v in inp.items()}
    pd = {k: torch.from_numpy(v.copy()) for k, v in inp.items()}
    metas = CenterHead.double_flip_decode(None, pd, [f"m{i}" for i in range(8)])
    for k, v in pd.items():
        out[f"out_{k}"] = v.numpy()
    out["metas"] = np.array(metas)
    save("double_flip.npz", **out)


def gen_swv_fragments():
    """The pieces of the geometry-aware head's Swin stage that DO execute in the reference (sw2votev4_util.py): ``window_partition`` /
    ``window_reverse`` (:28-39), ``MLP`` (:9-25), ``PatchEmbed`` (:390-419) and the whole of ``SwinTransformerBlock.forward`` (:125-188:
    norm1 -> zero padding to window multiples -> cyclic shift -> window partition -> attention -> reverse -> shift back -> crop ->
    residual -> norm2 -> MLP -> residual) -- the latter run as it stands in the reference with ONE substitution: its ``self.attn``
    (``WindowAttention``, whose constructor and forward cannot run: ``kernal_size``, ``.contiuous()``, ``torch.maixmum``, undefined ``B``)
    is replaced by the stand-in below, a masked uniform average over the window.  That is exactly what the real attention computes when
    q = k = 0, v = x, proj = identity and the vote / position MLPs are zero, so the oracle and the HIP kernels can be driven to the same
    function through their weights and everything AROUND the attention is pinned to reference code.  The shift mask handed to the
    block is ``oracle._swin_shift_mask`` (``BasicLayer.forward`` :262-276 builds it in a bool tensor and then subtracts bool tensors,
    which torch refuses -- another piece that cannot run).
    Inputs and weights are name-keyed seeded arrays (synth.seeded_normal / synth.load_filled, seed 77): the fixture holds OUTPUTS only.
    Channel count 256 / 4 heads as in the PARTNER head (the HIP window attention is built for head width 64)."""
    from det3d.models.bbox_heads.swin_utils import sw2votev4_util as U
    from oracle import polar_oracle as O
    SEED = 77
    B, H, W, C, ws = 2, 9, 11, 256, 7
    Hp = Wp = 14
    T = lambda name, *shape: torch.from_numpy(synth.seeded_normal("swv_frag." + name, shape, SEED))  # noqa: E731
    out = dict(dims=np.array([B, H, W, C, ws, Hp, Wp]), seed=np.int64(SEED))
    # ---- window_partition / window_reverse on a padded map (8 channels)
    xp = T("part_in", B, Hp, Wp, 8)
    win = U.window_partition(xp, ws)
    assert torch.equal(U.window_reverse(win, ws, Hp, Wp), xp)
    out["part_out"] = win.numpy()
    # ---- MLP (mlp_ratio 1, as the head builds it)
    m = U.MLP(in_features=C, hidden_features=C).eval()
    synth.load_filled(m, SEED)
    with torch.no_grad():
        out["mlp_out"] = m(T("mlp_in", 40, C)).numpy()
    # ---- PatchEmbed: 1 x 1 patches + LayerNorm, as SwinTransformer builds it for the head (:316-320)
    pe = U.PatchEmbed(patch_size=1, in_chans=2 * C, embed_dim=C, norm_layer=torch.nn.LayerNorm).eval()
    synth.load_filled(pe, SEED)
    with torch.no_grad():
        out["pe_out"] = pe(T("pe_in", B, 2 * C, H, W)).numpy()

    # ---- SwinTransformerBlock.forward around a stand-in attention
    class MaskedMeanAttention(torch.nn.Module):      # OURS (not reference code): softmax(mask) @ x, the real attention at q = k = 0, v = x
        def forward(self, x, mask=None, pos_embed=None, vote_embed=None):
            B_, N, _ = x.shape
            a = torch.zeros((B_, N, N))
            if mask is not None:
                nW = mask.shape[0]
                a = (a.view(B_ // nW, nW, N, N) + mask.unsqueeze(0)).view(-1, N, N)
            return a.softmax(dim=-1) @ x

    x, pos, vote = T("blk_x", B, H * W, C), T("blk_pos", B, H * W, 2), T("blk_vote", B, H * W, 3)
    for shift in (0, ws // 2):
        blk = U.SwinTransformerBlock.__new__(U.SwinTransformerBlock)      # the constructor builds WindowAttention and fails there
        torch.nn.Module.__init__(blk)
        blk.dim, blk.num_heads, blk.window_size, blk.shift_size, blk.mlp_ratio = C, 4, ws, shift, 1.0
        blk.norm1, blk.norm2 = torch.nn.LayerNorm(C), torch.nn.LayerNorm(C)
        blk.attn, blk.drop_path = MaskedMeanAttention(), torch.nn.Identity()
        blk.mlp = U.MLP(in_features=C, hidden_features=C)
        blk.H, blk.W = H, W
        blk.eval()
        synth.load_filled(blk, SEED + 1 + shift)
        mask = O._swin_shift_mask(Hp, Wp, ws, shift) if shift else None
        with torch.no_grad():
            out[f"blk_y_shift{shift}"] = blk(x, mask, pos, vote).numpy()
    save("swv_fragments.npz", **out)


REF_CONFIGS = ("configs/nusc/pp/polarstream_det_n_seg_1_sector.py", "configs/waymo/voxelnet/waymo_partner_36epoch.py",
               "configs/nusc/pp/polarstream/polarstream_det_n_seg_4_sector_trailing_edge.py",
               "configs/nusc/pp/polarstream/polarstream_det_n_seg_4_sector_bidirectional.py")


def gen_ref_configs():
    """the model / train_cfg / test_cfg / assigner values of the reference's config files as parsed by partner_amd.Config, as JSON
    (tuples as {"__tuple__": [...]}, loggers as {"__logger__": name}; test_host_api.py decodes them)"""
    import json
    import partner_amd as P

    def enc(v):
        if isinstance(v, dict):
            return {k: enc(x) for k, x in v.items()}
        if isinstance(v, list):
            return [enc(x) for x in v]
        if isinstance(v, tuple):
            return {"__tuple__": [enc(x) for x in v]}
        if isinstance(v, logging.Logger):
            return {"__logger__": v.name}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"{type(v).__name__} in a config value")

    out = {}
    for rel in REF_CONFIGS:
        c = P.Config.fromfile(os.path.join(ref_import.REFERENCE_ROOT, rel))
        out[rel] = {k: enc(c[k]) for k in ("model", "train_cfg", "test_cfg", "assigner") if k in c}
    path = os.path.join(HERE, "ref_configs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %-28s %8.1f KB" % ("ref_configs.json", os.path.getsize(path) / 1024))


if __name__ == "__main__":
    which = sys.argv[1:] or ["index", "hard", "reader", "full", "small", "heads", "setblock", "optim", "assign", "sweeps", "pillar_static", "seg_head", "e2e", "stream", "stream_bdcp", "augment", "double_flip", "swv_fragments", "ref_configs"]
    for w in which:
        globals()["gen_" + w]()
