"""The torch-CPU restatement of the proposal targets and the RoIHead's loss (tests/two_stage_train_ref.py, written from the header's
description) against the reference's own ProposalTargetLayer / assign_targets / get_loss run on recorded draws (two_stage_train.npz,
tests/golden/make_golden_two_stage_train.py).  No GPU."""
import numpy as np
import pytest
import torch

from tests import two_stage_train_ref as TR

CASES = [(bc, st, cs, False) for bc, st, cs in TR.CASES] + [(*TR.CASES[0], True)]


@pytest.fixture(scope="module")
def restated():
    """every case's restated targets, computed once"""
    return {c: TR.targets(TR.inputs(c[2], c[3]), TR.target_cfg(c[0], c[1])) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: TR.case_name(*c))
def test_restated_targets_match_the_reference(golden, restated, case):
    g, name, r = golden("two_stage_train.npz"), TR.case_name(*case), restated[case]
    np.testing.assert_array_equal(r["sampled_inds"].numpy(), g[f"{name}.sampled_inds"])
    for k in ("roi_labels", "reg_valid_mask"):
        assert r[k].dtype == torch.int64
        np.testing.assert_array_equal(r[k].numpy(), g[f"{name}.{k}"])
    for k in ("max_overlaps", "rois", "roi_scores", "gt_iou_of_rois", "roi_features", "gt_of_rois_src", "gt_of_rois", "rcnn_cls_labels"):
        ref = torch.from_numpy(np.asarray(g[f"{name}.{k}"])).float()
        assert r[k].shape == ref.shape, k
        err = float((r[k] - ref).abs().max() / max(float(ref.abs().max()), 1e-30))
        assert err < TR.REL, (k, err)
    inp = TR.inputs(case[2], case[3])
    for i in range(len(inp["rois"])):      # the picks are the rows the reference selected
        idx = r["sampled_inds"][i].long()
        np.testing.assert_array_equal(inp["rois"][i][idx].numpy(), g[f"{name}.rois"][i])
        np.testing.assert_array_equal(inp["roi_features"][i][idx].numpy(), g[f"{name}.roi_features"][i])


def test_branches_and_crafted_content(restated):
    """the four branches of the sampler are all taken, and by-class differs from all-class where the crafted ROI says so"""
    cfg = TR.TARGET_CFG
    quota = int(np.round(cfg["FG_RATIO"] * TR.M))
    mo = restated[(True, "roi_iou", 7, False)]["max_overlaps"]
    fg, hard, easy = (mo >= 0.55).sum(1), ((mo < 0.55) & (mo >= 0.1)).sum(1), (mo < 0.1).sum(1)
    assert fg[0] > quota and 0 < hard[0] < int((TR.M - quota) * cfg["HARD_BG_RATIO"]) and easy[0] > 0      # fg + both bg lists
    assert 0 < fg[1] < quota                                                                                  # fewer fg than the quota
    assert fg[2] == 0 and hard[2] == 0 and easy[2] == TR.R                                                    # background only, easy only
    f = restated[(True, "roi_iou", 7, True)]["max_overlaps"]
    assert bool((f >= 0.55).all())                                                                            # foreground only
    assert not torch.equal(mo[1], restated[(False, "roi_iou", 7, False)]["max_overlaps"][1])
    for thr in TR.THRESHOLDS:
        assert float((mo - thr).abs().min()) > TR.MARGIN
    labs = restated[(True, "cls", 7, False)]["rcnn_cls_labels"]
    assert set(labs.unique().tolist()) == {-1.0, 0.0, 1.0}


def test_largest_draw_stays_in_range():
    """the largest f32 below 1 against the largest list (all R slots): the pick is the list's last entry, never past it (for lengths
    whose f32 product rounds up to the length itself, 2^24 / 3 and more, the clamp of the contract does that)"""
    u = torch.tensor([1 - 2.0 ** -24], dtype=torch.float32)
    assert float(u) < 1.0 and int(TR.draw_index(u, TR.R)) == TR.R - 1 and int(TR.draw_index(u, 1 << 24)) == (1 << 24) - 1
    inp = TR.inputs(7)
    inp["u_bg"] = torch.full_like(inp["u_bg"], float(u))
    t = TR.targets(inp, TR.target_cfg(True))
    assert int(t["sampled_inds"].min()) >= 0 and int(t["sampled_inds"].max()) < TR.R
    easy2 = torch.nonzero(t["max_overlaps"][2] < 0.1).view(-1)
    assert bool((t["sampled_inds"][2] == int(easy2[-1])).all())      # sample 2: every pick is the LAST entry of its only list


@pytest.mark.parametrize("cs", [7, 9])
def test_restated_loss_matches_the_reference(golden, cs):
    g, name = golden("two_stage_train.npz"), TR.case_name(True, "roi_iou", cs)
    cls = torch.from_numpy(g[f"head{cs}_f32_rcnn_cls"]).double().requires_grad_()
    reg = torch.from_numpy(g[f"head{cs}_f32_rcnn_reg"]).double().requires_grad_()
    labels, enc, mask = (torch.from_numpy(np.asarray(g[f"{name}.{k}"])) for k in ("rcnn_cls_labels", "gt_of_rois", "reg_valid_mask"))
    w = TR.LOSS_CFG["LOSS_WEIGHTS"]
    loss = TR.roi_loss(cls, reg, labels, enc, mask, TR.code_weights(cs), w["rcnn_cls_weight"], w["rcnn_reg_weight"])
    ref = torch.from_numpy(g[f"head{cs}_f32_loss"]).double()
    for a, b in zip([v.detach() for v in loss], ref):
        assert abs(float(a) - float(b)) <= 3e-4 * abs(float(b)), (float(a), float(b))
