"""The torch restatement of the hard-voxel PillarFeatureNet in training form (tests/pfn_static_train_ref.py) on the CPU: pinned by the
reference's own module (tests/golden/pfn_static_train.npz, written by tests/golden/make_golden_pfn_static_train.py), equal to the oracle's
eval form when the BatchNorm layers use their running buffers, and indifferent to which of several equal slots the maximum selects."""
import os

import numpy as np
import pytest
import torch

from tests import pfn_static_train_ref as R

F32, F64 = torch.float32, torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pfn_static_train.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_restatement_matches_the_reference_module(golden):
    """float32 against float32: the restatement issues the reference's own torch calls"""
    case = R.draw_case(R.GOLDEN_CASE, seed=7)
    for k in ("voxels", "num_points", "coors", "d_out"):
        np.testing.assert_array_equal(case[k], golden[k])
    for k, v in case["sd"].items():
        np.testing.assert_array_equal(np.array(v), golden["sd " + k])
    res = R.run(case, F32)
    np.testing.assert_allclose(res["out"].numpy(), golden["out"], rtol=0, atol=1e-6 * float(np.abs(golden["out"]).max()))
    n_grads = 0
    for k in case["sd"]:
        if k.endswith(R.PARAM_KEYS):
            ref = golden["d " + k]
            np.testing.assert_allclose(res["d " + k].numpy(), ref, rtol=0, atol=1e-5 * float(np.abs(ref).max()), err_msg=k)
            n_grads += 1
        elif k.endswith("num_batches_tracked"):
            assert int(res[k]) == int(golden["after " + k]) == int(case["sd"][k]) + 1
        else:
            np.testing.assert_allclose(res[k].numpy(), golden["after " + k], rtol=1e-6, atol=1e-7, err_msg=k)
            assert not np.array_equal(golden["after " + k], golden["sd " + k])
    assert n_grads == 6


def test_float64_run_agrees_with_the_golden_to_float32_accuracy(golden):
    case = R.draw_case(R.GOLDEN_CASE, seed=7)
    res = R.run(case, F64)
    assert float((res["out"] - torch.from_numpy(golden["out"]).double()).abs().max()) < 1e-3
    # the saved statistics are the ones the normalisation used
    vox, num, coors, sd = R.tensors(case, F64)
    z0 = R.decorate(vox, num, coors, False) @ sd["pfn_layers.0.linear.weight"].t()
    assert torch.allclose(res["mean0"], z0.reshape(-1, z0.shape[-1]).mean(0))
    n = z0.shape[0] * z0.shape[1]
    rv = (1 - R.MOMENTUM) * torch.from_numpy(case["sd"]["pfn_layers.0.norm.running_var"]).double() + \
        R.MOMENTUM * z0.reshape(n, -1).var(0, unbiased=True)
    assert torch.allclose(res["pfn_layers.0.norm.running_var"], rv)


@pytest.mark.parametrize("name", ["one_layer_distance", "wide_layer1", "all_single"])
def test_eval_mode_equals_the_oracle(name):
    from oracle import polar_oracle as O
    case = R.draw_case(R.CASES[name], seed=3)
    vox, num, coors, sd = R.tensors(case, F64)
    with torch.no_grad():
        x = R.decorate(vox, num, coors, case["spec"]["dist"])
        got, _ = R.pfn_forward(sd, x, case["n_layers"], train=False)
        want = O.pillar_feature_net_static({k: v.detach() for k, v in sd.items()}, "", vox, num, coors, R.WAYMO_VOXEL, R.WAYMO_RANGE,
                                           with_distance=case["spec"]["dist"], eps=R.EPS)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) < 1e-10
    assert int(sd["pfn_layers.0.norm.num_batches_tracked"]) == int(case["sd"]["pfn_layers.0.norm.num_batches_tracked"])


@pytest.mark.parametrize("name", ["waymo_offset", "one_layer_distance", "all_single"])
def test_slot_order_changes_no_parameter_gradient(name):
    """the tie argument of the backward: equal slots are rows with identical inputs (or the value 0), so the parameter gradients do not
    depend on which of them the maximum selects -- permute the slots inside every pillar, padded slots to the front included"""
    case = R.draw_case(R.CASES[name], seed=5)
    V, P = case["spec"]["V"], case["spec"]["P"]
    base = R.run(case, F64)
    g = np.random.Generator(np.random.PCG64(9))
    perms = {"reversed": np.tile(np.arange(P)[::-1], (V, 1)), "random": np.stack([g.permutation(P) for _ in range(V)])}
    assert (case["num_points"] < P).any()      # reversed: the padded slots come first, the first maximum is another row
    for tag, perm in perms.items():
        res = R.run(case, F64, slot_perm=perm)
        for k, ref in base.items():
            if k.startswith("d ") or k == "out":
                err = float((res[k] - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
                assert err < 1e-11, (tag, k, err)
