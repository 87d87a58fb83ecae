"""The hard-voxel PillarFeatureNet in TRAINING form, restated in torch (any dtype, CPU): ``PillarFeatureNet.forward`` +
``PFNLayer.forward_static`` (det3d/models/readers/pillar_encoder.py:129-169, 49-61) with the module in train mode.  The float64 run is the
reference of tests/test_hip_pfn_static_train.py and of the reader inside tests/test_hip_train_centerpoint.py, the float32 run their error
unit; tests/golden/pfn_static_train.npz (the reference's own module) pins it in tests/test_pfn_static_train_cpu.py.

Per layer  z = x W^T,  BatchNorm1d over all V*P rows (the padded slots included; biased variance in the normalisation, the unbiased one into
``running_var``),  ReLU,  max over the P slots;  layer 1 reads [y0_p, max_p y0] in every slot.  Inputs are continuous draws, so equal slots
arise only as rows with identical inputs (the padded slots) or at the value 0, where the choice of the maximum's slot changes no gradient.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

WAYMO_RANGE, WAYMO_VOXEL = [-74.88, -74.88, -2.0, 74.88, 74.88, 4.0], [0.32, 0.32, 6.0]
PARAM_KEYS = ("linear.weight", "norm.weight", "norm.bias")
BUFFER_KEYS = ("norm.running_mean", "norm.running_var", "norm.num_batches_tracked")
EPS, MOMENTUM = 1e-3, 0.01      # PFNLayer's norm_cfg default: BN1d(eps=1e-3, momentum=0.01)

# name -> V, P, F, num_filters, with_distance, how num_points is drawn
CASES = {
    "waymo_offset": dict(V=301, P=20, F=5, filters=(64, 64), dist=False, num="mixed"),
    "smallest": dict(V=1, P=2, F=5, filters=(64, 64), dist=False, num="full"),
    "one_layer_distance": dict(V=77, P=5, F=5, filters=(64,), dist=True, num="mixed"),
    "wide_layer1": dict(V=150, P=12, F=4, filters=(64, 128), dist=False, num="mixed"),
    "all_full": dict(V=130, P=9, F=5, filters=(64, 64), dist=False, num="full"),
    "all_single": dict(V=130, P=9, F=5, filters=(64, 64), dist=False, num="one"),
}
GOLDEN_CASE = dict(V=90, P=8, F=5, filters=(64, 64), dist=False, num="mixed")


def layer_channels(nin, filters):
    """[(in, out)] per PFN layer: every layer but the last has half its filter count (the other half is the repeated maximum)"""
    chans, cin = [], nin
    for i, f in enumerate(filters):
        cout = f if i == len(filters) - 1 else f // 2
        chans.append((cin, cout))
        cin = f
    return chans


def draw_case(spec, seed=0, canvas=(468, 468), batch=2):
    """-> dict of numpy inputs, parameters ``sd`` (float32, keys of PillarFeatureNet.state_dict()) and the seeded output gradient.  Pillars
    sit in distinct cells of the Waymo pillar grid (x, y over +-74.88 m at 0.32 m), their points inside the cell; padded slots are zero."""
    g = np.random.Generator(np.random.PCG64(1000 + seed))
    V, P, Fe = spec["V"], spec["P"], spec["F"]
    W, H = canvas
    cells = g.choice(batch * H * W, V, replace=False)
    b, y, x = cells // (H * W), (cells // W) % H, cells % W
    coors = np.stack([b, np.zeros_like(b), y, x], 1).astype(np.int32)
    num = dict(full=np.full(V, P), one=np.ones(V, np.int64), mixed=g.integers(1, P + 1, V))[spec["num"]]
    if spec["num"] == "mixed" and V >= 4:
        num[:2], num[2] = P, 1
    vx, vy = WAYMO_VOXEL[:2]
    vox = np.zeros((V, P, Fe), np.float32)
    vox[..., 0] = WAYMO_RANGE[0] + (x[:, None] + g.random((V, P))) * vx
    vox[..., 1] = WAYMO_RANGE[1] + (y[:, None] + g.random((V, P))) * vy
    vox[..., 2] = g.uniform(-2, 4, (V, P))
    vox[..., 3:] = g.random((V, P, Fe - 3))
    vox *= (np.arange(P)[None, :] < num[:, None])[..., None]
    nin = Fe + 5 + int(spec["dist"])
    sd = {}
    for i, (cin, cout) in enumerate(layer_channels(nin, spec["filters"])):
        p = f"pfn_layers.{i}."
        sd[p + "linear.weight"] = (g.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
        sd[p + "norm.weight"] = (g.uniform(0.5, 1.5, cout) * np.where(g.random(cout) < 0.1, -1.0, 1.0)).astype(np.float32)
        sd[p + "norm.bias"] = (0.3 * g.standard_normal(cout)).astype(np.float32)
        sd[p + "norm.running_mean"] = (0.1 * g.standard_normal(cout)).astype(np.float32)
        sd[p + "norm.running_var"] = g.uniform(0.5, 1.5, cout).astype(np.float32)
        sd[p + "norm.num_batches_tracked"] = np.array(3 + i, np.int64)
    d_out = g.standard_normal((V, spec["filters"][-1])).astype(np.float32)
    return dict(spec=dict(spec), voxels=vox, num_points=num.astype(np.int32), coors=coors, sd=sd, d_out=d_out, canvas=(batch, H, W),
                n_layers=len(spec["filters"]))


def decorate(voxels, num_points, coors, with_distance, voxel_size=WAYMO_VOXEL, pc_range=WAYMO_RANGE):
    """pillar_encoder.py:137-164: [features, xyz - mean (the sum over all P slots / num_points), xy - pillar centre(, |xyz|)], padded slots zeroed"""
    vx, vy = voxel_size[0], voxel_size[1]
    xo, yo = vx / 2 + pc_range[0], vy / 2 + pc_range[1]
    dt = voxels.dtype
    mean = voxels[:, :, :3].sum(dim=1, keepdim=True) / num_points.to(dt).view(-1, 1, 1)
    center = torch.zeros_like(voxels[:, :, :2])
    center[:, :, 0] = voxels[:, :, 0] - (coors[:, 3].to(dt).unsqueeze(1) * vx + xo)
    center[:, :, 1] = voxels[:, :, 1] - (coors[:, 2].to(dt).unsqueeze(1) * vy + yo)
    parts = [voxels, voxels[:, :, :3] - mean, center]
    if with_distance:
        parts.append(torch.norm(voxels[:, :, :3], 2, 2, keepdim=True))
    x = torch.cat(parts, dim=-1)
    mask = (torch.arange(voxels.shape[1])[None, :] < num_points[:, None]).to(dt).unsqueeze(-1)
    return x * mask


def pfn_forward(sd, x, n_layers, train=True, eps=EPS, momentum=MOMENTUM):
    """the PFN layers on decorated rows ``x`` (V, P, nin).  ``sd``: tensors of x's dtype (the running buffers are updated IN PLACE in train mode).
    -> (features (V, C_last), [(batch mean, inverse standard deviation)] per layer)"""
    stats = []
    for i in range(n_layers):
        p = f"pfn_layers.{i}."
        z = F.linear(x, sd[p + "linear.weight"])
        flat = z.reshape(-1, z.shape[-1])
        stats.append((flat.mean(0).detach(), 1.0 / torch.sqrt(flat.var(0, unbiased=False).detach() + eps)))
        y = F.batch_norm(z.permute(0, 2, 1).contiguous(), sd[p + "norm.running_mean"], sd[p + "norm.running_var"], sd[p + "norm.weight"],
                         sd[p + "norm.bias"], training=train, momentum=momentum, eps=eps).permute(0, 2, 1).contiguous()
        if train:
            sd[p + "norm.num_batches_tracked"] += 1
        y = F.relu(y)
        ymax = torch.max(y, dim=1, keepdim=True)[0]
        x = ymax if i == n_layers - 1 else torch.cat([y, ymax.repeat(1, y.shape[1], 1)], dim=2)
    return x.squeeze(1), stats


def tensors(case, dtype, count=None):
    """-> (voxels, num_points, coors, sd) as torch tensors of ``dtype`` (parameters with requires_grad); ``count``: the first rows only"""
    n = case["spec"]["V"] if count is None else count
    sd = {}
    for k, v in case["sd"].items():
        t = torch.from_numpy(np.array(v))
        sd[k] = t.clone() if k.endswith("num_batches_tracked") else t.to(dtype).clone()
        if k.endswith(PARAM_KEYS):
            sd[k].requires_grad_(True)
    return torch.from_numpy(case["voxels"][:n]).to(dtype), torch.from_numpy(case["num_points"][:n]).long(), torch.from_numpy(case["coors"][:n]).long(), sd


def run(case, dtype, count=None, slot_perm=None):
    """forward in train mode + autograd for the seeded ``d_out`` -> dict: out, mean{i}, rstd{i}, the buffers after the forward and the six (three)
    parameter gradients, keyed like the state dict.  ``slot_perm``: (V, P) permutation of the slots inside every pillar, applied to the
    decorated rows (padded slots may move anywhere)."""
    vox, num, coors, sd = tensors(case, dtype, count)
    x = decorate(vox, num, coors, case["spec"]["dist"])
    if slot_perm is not None:
        x = torch.gather(x, 1, torch.from_numpy(slot_perm).long()[:, :, None].expand_as(x))
    out, stats = pfn_forward(sd, x, case["n_layers"])
    out = out.reshape(vox.shape[0], -1)
    d_out = torch.from_numpy(case["d_out"][:vox.shape[0]]).to(dtype)
    out.backward(d_out)
    res = {"out": out.detach()}
    for i, (m, r) in enumerate(stats):
        res[f"mean{i}"], res[f"rstd{i}"] = m, r
    for k, v in sd.items():
        if k.endswith(PARAM_KEYS):
            res["d " + k] = v.grad
        else:
            res[k] = v.detach()
    return res
