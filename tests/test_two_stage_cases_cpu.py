"""The conditions that tests/test_hip_two_stage_kernels.py puts on its inputs, asserted without a GPU for every generator of
tests/two_stage_cases.py: margins, list sizes on the intended side of every branch, tie placements, redraw caps and FACTOR * e32 < REL;
and the float64 evaluation of the restatements against their float32 form on the golden inputs.  Needs `make -C oracle`."""
import numpy as np
import pytest
import torch

from tests import two_stage_cases as K
from tests import two_stage_ref as TR2
from tests import two_stage_train_ref as TR

REL, FACTOR, F64 = TR.REL, K.FACTOR, torch.float64


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / max(float(ref.double().abs().max()), 1e-30))


# ------------------------------------------------------------------------------------------------ the float64 twins on the golden inputs
@pytest.mark.parametrize("tag", ["A", "B"])
def test_float64_gather_agrees_with_float32_on_the_golden_inputs(tag):
    k = TR2.GATHER_CASES[tag]
    boxes, scores, labels, counts, bev = TR2.gather_inputs(tag)
    r32 = TR2.gather(boxes, scores, labels, counts, bev, k["num_point"], k["cols"], k["max_rois"])
    r64 = TR2.gather(boxes.double(), scores, labels, counts, bev.double(), k["num_point"], k["cols"], k["max_rois"])
    assert r64[3].dtype == F64 and torch.equal(r64[0].float(), r32[0]) and torch.equal(r64[1], r32[1]) and torch.equal(r64[2], r32[2])
    assert rel_err(r32[3], r64[3]) < REL
    cls, reg = TR2.refine_inputs(k["cols"])
    f32 = TR2.refine(r32[0], r32[1], r32[2], counts, cls, reg)
    f64 = TR2.refine(r32[0].double(), r32[1].double(), r32[2], counts, cls.double(), reg.double())
    assert f64[0].dtype == F64 and rel_err(f32[0], f64[0]) < REL and rel_err(f32[1], f64[1]) < REL and torch.equal(f32[2], f64[2])


@pytest.mark.parametrize("by_class,score_type,cs", TR.CASES)
def test_float64_targets_agree_with_float32_on_the_golden_inputs(by_class, score_type, cs):
    inp, cfg = TR.inputs(cs), TR.target_cfg(by_class, score_type)
    mo, ga = TR.max_iou(inp["rois"], inp["roi_labels"], inp["gt"], by_class)
    t32, t64 = TR.targets(inp, cfg, mo, ga), TR.targets(inp, cfg, mo, ga, dtype=F64)
    for key in TR.TARGET_KEYS:
        if key in ("gt_of_rois", "rcnn_cls_labels"):
            assert t64[key].dtype == F64 and rel_err(t32[key], t64[key]) < REL, key
        else:
            assert t64[key].dtype == t32[key].dtype and torch.equal(t64[key], t32[key]), key


# ------------------------------------------------------------------------------------------------ gather, refine, loss
def test_gather_cases():
    assert bool(K.off_integers(np.asarray(TR2.CRAFTED), 5).all()), "a crafted box has a sample point on a cell border"
    cases = [K.gather_case(s) for s in K.GATHER_CASES] + [K.gather_case(*K.GATHER_NEGATIVE)]
    for k in cases:
        b, h, w, c, p, cols, cap, r = k["shape"]
        assert FACTOR * k["e32"] < REL, (k["shape"], k["e32"])
        assert k["redrawn"] <= max(1, sum(k["eff"]) // 50), (k["shape"], k["redrawn"])
        for i, n in enumerate(k["eff"]):
            assert bool(torch.isnan(k["boxes"][i, n:]).all()) and bool(torch.isnan(k["scores"][i, n:]).all())
            if n:
                assert bool(K.off_integers(k["boxes"][i, :n].numpy()[:, list(range(6)) + [cols - 1]], 5).all())
    counts = [n for k in cases for n in zip(k["counts"].tolist(), k["eff"])]
    assert (508, 501) in counts and (0, 0) in counts and (-3, 0) in counts and (501 + 7, 501) in counts and (12, 12) in counts
    big = K.gather_case((2, 24, 40, 260, 5, 9, 12, 12))
    x, y = K.map_coords(big["boxes"][0, :12].double(), 5)
    assert bool((x < 0).any()) and bool((x > 40).any()) and bool((y < 0).any()) and bool((y > 24).any())      # points on every side of the map
    null = big["scale"] != big["ref64"][3].abs().amax(-1)
    assert 0 < int(null.sum()) < 21                              # some slots lie wholly beside the map, most do not


@pytest.mark.parametrize("cs", [7, 9])
def test_refine_cases(cs):
    seen = []
    for shape in K.REFINE_CASES:
        k = K.refine_case(shape, cs)
        assert FACTOR * max(K.refine_e32(shape, cs)) < REL
        seen += list(zip(k["counts"].tolist(), k["eff"]))
        for i, n in enumerate(k["eff"]):
            assert bool(torch.isnan(k["rois"][i, n:]).all())
    assert set(seen) >= {(0, 0), (500, 500), (505, 500), (-1, 0)}
    k = K.refine_case((3, 500), cs)
    rot = k["rois"][1, :, 6]
    assert {int(v) for v in torch.floor(torch.remainder(rot, 2 * np.pi) / (np.pi / 2))} == {0, 1, 2, 3} and float(rot.abs().max()) > 2 * np.pi
    assert float(k["cls"].view(3, 500)[1, 0]) == 100 and float(k["cls"].view(3, 500)[1, 1]) == -100 and float(k["roi_scores"][1, 2]) == 0


def test_loss_cases():
    assert {c[0] for c in K.LOSS_CASES} == {1, 255, 256, 257, 512, 1000} and {c[2] for c in K.LOSS_CASES} == {"mixed", "all", "none", "beyond256", "below256"}
    for case in K.LOSS_CASES:
        k = K.loss_case(case)
        assert FACTOR * K.loss_e32(case) < REL, (case, k["e32"])
        lab, mask = k["labels"], k["mask"]
        if case[2] == "mixed" and case[0] > 4:
            assert bool((lab == 0).any()) and bool((lab == 1).any()) and bool((lab == -1).any()) and bool(((lab > 0) & (lab < 1)).any())
            assert 0 < int(mask.sum()) < len(mask)
        if case[2] == "beyond256":
            assert not mask[:256].any() and bool(mask[256:].all()) and bool((lab[:256] == -1).all())
        if case[2] == "below256":
            assert not mask[256:].any() and bool(mask[:256].all()) and bool((lab[256:] == -1).all())


# ------------------------------------------------------------------------------------------------ max IoU
@pytest.mark.parametrize("shape", K.IOU_CASES, ids=str)
def test_iou_cases(shape):
    geo = K.iou_geometry(shape)
    b, r, n = shape
    assert geo["replaced"] <= K.REDRAW_CAP * r + (r < 100), geo["replaced"]
    rois, labels, gt = geo["rois"], torch.from_numpy(geo["labels"]), torch.from_numpy(geo["gt"])
    m = K.iou32(rois[0], geo["gt"][0, :geo["kept"]])
    live = geo["live"]
    for by_class in (True, False):                               # none remains
        assert float(K.competing_gap(m, labels[0], gt[0], by_class)[:live].min()) >= K.IOU_GAP
    for sign in (-1, 1):
        moved = K.shifted(rois[0], sign)
        assert bool((moved[:live, 0] != rois[0, :live, 0]).all())
        assert float((K.iou32(moved, geo["gt"][0, :geo["kept"]]) - m).abs()[:live].max()) <= REL
    assert TR.kept_rows(gt[0]) == geo["kept"]
    by_cls, all_cls = K.iou_case(shape, True, 7), K.iou_case(shape, False, 7)
    for k in (by_cls, all_cls, K.iou_case(shape, True, 9)):
        ga, mo = k["gt_assignment"], k["max_overlaps"]
        for s, row in geo["slots"]["best"]:
            assert int(ga[0, s]) == row and float(mo[0, s]) > 0.5
        for s, _ in geo["slots"]["far"]:
            assert float(mo[0, s]) == 0
    if n >= 129:
        assert geo["kept"] == 129 and not gt[0, K.ZERO_ROW].any() and not gt[0, 129].any() and bool(gt[0, 128].any())
        assert [row for _, row in geo["slots"]["best"]] == list(K.BEST_ROWS)
        for k in (by_cls, all_cls, K.iou_case(shape, True, 9)):
            ga, mo, g = k["gt_assignment"], k["max_overlaps"], k["gt"]
            for lo, hi in K.TWINS:                                   # bit-identical rows: the lower index wins, for an ROI drawn at either
                assert torch.equal(g[0, lo], g[0, hi]) and (hi - lo == 64 or (hi - lo) % 64)
                for what, row in (("twin", lo), ("twin_hi", hi)):
                    s = [s for s, kk in geo["slots"][what] if kk == row][0]
                    assert int(ga[0, s]) == lo and float(mo[0, s]) > 0.1
            assert not mo[1].any() and not ga[1].any()               # the sample without gt
            assert not k["rois"][0, geo["live"]:].any() and not mo[0, geo["live"]:].any()      # padding slots
        for s, _ in geo["slots"]["noclass"]:                     # no gt of class 4: (0, 0) by class, its neighbour otherwise
            assert float(by_cls["max_overlaps"][0, s]) == 0 and int(by_cls["gt_assignment"][0, s]) == 0 and float(all_cls["max_overlaps"][0, s]) > 0.5
        far = [s for s, _ in geo["slots"]["far"]]
        assert {int(v) for v in by_cls["gt_assignment"][0, far]} == {0, 1, 2} and not all_cls["gt_assignment"][0, far].any()
        assert int(by_cls["gt_assignment"][0, geo["live"]]) == K.ZERO_ROW      # a zero ROI (label 0) meets the zero gt row (class 0)
    else:
        assert geo["kept"] == 65 and int(by_cls["gt_assignment"][0, 0]) == 64


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("name", list(K.SAMPLER_CASES))
def test_sampler_cases(name):
    (b, r, n, m, f), score_type, cs, sizes = K.SAMPLER_CASES[name]
    k = K.sampler_case(name)
    assert FACTOR * max(K.sampler_e32(name).values()) < REL
    assert bool(K.off_thresholds(k["max_overlaps"]).all())
    assert k["redrawn"] <= 0.25 * b * r, k["redrawn"]             # about one ROI in ten needs a redraw
    for i, (nf, nh) in enumerate(sizes):
        assert K.lists_of(k["max_overlaps"][i]) == (nf, nh, r - nf - nh)
    u_fg, u_bg = k["inp"]["u_fg"], k["inp"]["u_bg"]
    assert float(u_fg[0, 1]) == float(u_fg[0, 3]) and float(u_bg[0, 0]) == 0
    if m >= 4:
        assert float(u_bg[0, 1]) == K.U_MAX == float(u_bg[0, m - 1]) < 1
    inds = k["ref32"]["sampled_inds"]
    assert tuple(inds.shape) == (b, m) and int(inds.min()) >= 0 and int(inds.max()) < r


def test_sampler_cases_take_every_branch():
    quota = lambda name: int(np.round(0.5 * K.SAMPLER_CASES[name][0][3]))      # noqa: E731
    assert quota("quota_2.5") == 2 and quota("quota_1.5") == 2 and quota("one_row") == 0
    prod = K.sampler_case("production")
    fg0 = torch.nonzero(prod["max_overlaps"][0] >= 0.55).view(-1)
    assert int(fg0.min()) < 256 <= int(fg0.max())                # foreground in both scan rounds
    (nf0, nh0), (nf1, nh1) = prod["sizes"]
    assert nf0 > 64 and nh0 < int((128 - 64) * 0.8) and nf1 < 64 and nh1 > int((128 - nf1) * 0.8)
    inds = prod["ref32"]["sampled_inds"][0, :64].tolist()        # the duplicated keys: list position 1 before 3, both picked
    assert inds.index(int(fg0[1])) + 1 == inds.index(int(fg0[3]))
    second = K.sampler_case("second_round")
    assert int(torch.nonzero(second["max_overlaps"][0] >= 0.55).view(-1).max()) == 256 and K.SAMPLER_CASES["second_round"][0][3] > 256
    rank = K.sampler_case("rank_strides")
    fg = torch.nonzero(rank["max_overlaps"][0] >= 0.55).view(-1)
    inds = rank["ref32"]["sampled_inds"][0, :64].tolist()
    assert len(fg) > 300 and inds.index(int(fg[2])) + 1 == inds.index(int(fg[260]))      # equal keys two strides apart
    assert K.lists_of(K.sampler_case("all_foreground")["max_overlaps"][0]) == (600, 0, 0)
    lim = K.SAMPLER_CASES["limits"][0]
    assert lim[1] == lim[3] == 2048
    kinds = {name: tuple(bool(v) for v in K.lists_of(K.sampler_case(name)["max_overlaps"][0])) for name in K.SAMPLER_CASES}
    assert kinds["no_foreground"] == (False, True, True) and kinds["hard_only"] == (False, True, False)
    assert kinds["fg_and_easy"] == (True, False, True) and kinds["fg_and_hard"] == (True, True, False)
    assert {K.SAMPLER_CASES[n][1] for n in K.SAMPLER_CASES} == {"roi_iou", "cls"} and {K.SAMPLER_CASES[n][2] for n in K.SAMPLER_CASES} == {7, 9}
    labels = K.sampler_case("production_cls9")["ref32"]["rcnn_cls_labels"]
    assert bool((labels == -1).any()) and bool((labels == 1).any()) and bool((labels == 0).any())
    soft = prod["ref32"]["rcnn_cls_labels"]
    assert bool(((soft > 0) & (soft < 1)).any())
