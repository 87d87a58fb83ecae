#!/usr/bin/env python3
"""Golden vectors of the hard-voxel reader in TRAIN mode: runs the REFERENCE's ``PillarFeatureNet(num_input_features=5, num_filters=(64, 64),
voxel_size=Waymo pillar, pc_range=Waymo pillar).train()`` (models/readers/pillar_encoder.py:74-169, 19-61), imported through ref_import.py,
on the CPU in float32 and stores what it computes in ``pfn_static_train.npz``.

Container-only: ``python tests/golden/make_golden_pfn_static_train.py``.  Data only.  Inputs and parameters are the seeded draw
``tests.pfn_static_train_ref.draw_case(GOLDEN_CASE, seed=7)`` (stored too: ``voxels``, ``num_points``, ``coors``, ``d_out`` and every state-dict
entry as ``sd {key}``).  Results: ``out`` (V, 64), ``d {parameter key}`` = the autograd gradients of the six parameters for ``d_out``, and the three
buffers of each layer after ONE forward as ``after {key}``.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_import  # noqa: E402
from tests import pfn_static_train_ref as R  # noqa: E402

torch.set_num_threads(8)
det3d = ref_import.import_reference()
from det3d.models.readers.pillar_encoder import PillarFeatureNet  # noqa: E402


def main():
    case = R.draw_case(R.GOLDEN_CASE, seed=7)
    spec = case["spec"]
    net = PillarFeatureNet(num_input_features=spec["F"], num_filters=tuple(spec["filters"]), with_distance=spec["dist"], voxel_size=R.WAYMO_VOXEL,
                           pc_range=R.WAYMO_RANGE)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in case["sd"].items()}, strict=True)
    net.train()
    for layer in net.pfn_layers:
        assert layer.norm.eps == R.EPS and layer.norm.momentum == R.MOMENTUM
    out = net(torch.from_numpy(case["voxels"]), torch.from_numpy(case["num_points"]), torch.from_numpy(case["coors"]))
    out.backward(torch.from_numpy(case["d_out"]))
    res = dict(voxels=case["voxels"], num_points=case["num_points"], coors=case["coors"], d_out=case["d_out"], out=out.detach().numpy())
    for k, v in case["sd"].items():
        res["sd " + k] = np.array(v)
    for k, p in net.named_parameters():
        res["d " + k] = p.grad.numpy()
    for k, b in net.named_buffers():
        res["after " + k] = b.detach().numpy()
    assert sorted(k for k in res if k.startswith("d ")) == sorted("d " + k for k in case["sd"] if k.endswith(R.PARAM_KEYS))
    path = os.path.join(HERE, "pfn_static_train.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print("wrote pfn_static_train.npz %8.1f KB," % (size / 1024), len(res), "arrays; out", res["out"].shape)
    assert size < 1024 * 1024


if __name__ == "__main__":
    main()
