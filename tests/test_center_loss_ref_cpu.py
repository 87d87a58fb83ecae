"""CPU checks of tests/center_loss_ref.py: the float64 restatement against ``oracle.polar_oracle.center_loss`` run in float64 (value and
autograd gradients, 1e-12 relative), the builder's two conditions on every case of the GPU file's list, and that the list reaches the
paths of csrc/loss.hip it is there for."""
import numpy as np
import pytest
import torch

from tests.center_loss_ref import CASES, GATE_HI, GATE_LO, center_loss_ref, check_conditions, get_case

BOX_NAMES = {5: ("reg", "height", "dim", "vel", "rot"), 4: ("reg", "height", "dim", "rot")}


def oracle_f64(case, grad_scale):
    from oracle import polar_oracle as O
    names = BOX_NAMES[len(case.boxes)]
    preds = {k: v.double().clone().requires_grad_(True) for k, v in zip(names, case.boxes)}
    preds["hm"] = case.hm.double().clone().requires_grad_(True)
    loss = O.center_loss(preds, case.hm_t.double(), case.ind, case.mask, case.cat, case.anno.double(), code_weights=case.code_weights,
                         weight=case.weight)
    (loss["det_loss"] * grad_scale).backward()
    out = np.array([float(loss[k].detach()) for k in ("det_loss", "hm_loss", "loc_loss", "num_positive")]
                   + [float(v) for v in loss["loc_loss_elem"].detach()])
    g = lambda v: (torch.zeros_like(v) if v.grad is None else v.grad).numpy()  # noqa: E731
    return dict(out=out, d_hm=g(preds["hm"]), d_boxes=[g(preds[k]) for k in names])


@pytest.mark.parametrize("name", ["no_positives", "stacked", "partial_wave_novel8"])
def test_restatement_equals_the_oracle_in_float64(name):
    """no_positives: num_pos == 0; stacked: triple duplicates, mixed classes in a cell, slots that are not live colliding with live
    ones (at cell 0 of class 0 and at the triple's cell); partial_wave_novel8: with_vel=False"""
    case = get_case(name)
    live = case.mask.bool()
    if name == "no_positives":
        assert not bool(live.any()) and bool((case.ind != 0).any())
    if name == "stacked":
        b = 4
        assert case.ind[b, 1] == case.ind[b, 3] == case.ind[b, 5] == case.ind[b, 4] == case.ind[b, 2] != 0
        assert case.cat[b, 1] == case.cat[b, 3] == case.cat[b, 5] == case.cat[b, 2] != case.cat[b, 4]
        assert live[b, [1, 3, 4, 5, 6]].all() and not live[b, [0, 2, 7]].any()
        assert case.ind[b, 6] == 0 and case.cat[b, 6] == 0 and case.ind[b, 0] == 0 and case.cat[b, 0] == 0
    if name == "partial_wave_novel8":
        assert not case.with_vel and case.anno.shape[2] == 8 and len(case.boxes) == 4
    want = oracle_f64(case, 0.25)
    got = center_loss_ref(*case.ref_args(), grad_scale=0.25)
    assert got["out"][3] == want["out"][3] == float(live.sum())
    assert np.abs(got["out"] - want["out"]).max() <= 1e-12 * np.abs(want["out"][:3]).max()
    assert np.abs(got["d_hm"] - want["d_hm"]).max() <= 1e-12 * np.abs(want["d_hm"]).max()
    for a, b_ in zip(got["d_boxes"], want["d_boxes"]):
        assert a.shape == b_.shape and np.abs(a - b_).max() <= 1e-12 * np.abs(want["d_boxes"][0]).max()
    if name == "no_positives":
        assert got["out"][1] > 0 and got["out"][2] == 0 and not any(a.any() for a in got["d_boxes"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_builder_conditions(name):
    """no logit next to the clamp gate, saturated cells exactly at +-30 / +-100, ties exact in float32 and in float64"""
    case = get_case(name)
    check_conditions(case)
    a = case.hm.double().abs()
    assert not bool(((a > GATE_LO) & (a < GATE_HI)).any())
    # the sides of the gate agree between the two precisions
    for dt in (torch.float32, torch.float64):
        s = torch.sigmoid(case.hm.to(dt))
        inside = (s >= 1e-4) & (s <= 1 - 1e-4)
        assert torch.equal(inside, a < 9.2)


def test_case_list_reaches_the_paths():
    """what the review reads off the case table, asserted: the launch caps, the 256-thread strides, the partial wave, the full list,
    mult >= 3, a live object at cell 0 of class 0 behind a slot that is not live, saturation at live and background cells, ties"""
    def dims(name):
        c = get_case(name)
        b, ncls, h, w = c.hm.shape
        return c, b, ncls, h, w, c.ind.shape[1]
    c, b, ncls, h, w, m = dims("grid_stride")
    assert b * ncls * h * w > 1024 * 256 and b * h * w * ((ncls + 3) // 4 * 4) > 4096 * 256
    c, b, ncls, h, w, m = dims("tiny")
    assert (b, ncls, h, w, m) == (1, 1, 4, 4, 1) and int(c.mask.sum()) == 1
    c, b, ncls, h, w, m = dims("partial_wave")
    assert m % 64 != 0 and ncls == 3 and bool(c.mask[:, 64:].any())
    c, b, ncls, h, w, m = dims("strided_objects")
    assert m > 256 and int(c.mask[0].sum()) > 256 and int(c.mask[1].sum()) == 0 and bool(c.mask[0, 256:].any())
    key = (c.ind[0] * ncls + c.cat[0])[c.mask[0].bool()]
    assert int(torch.unique(key, return_counts=True)[1].max()) >= 3
    c, b, ncls, h, w, m = dims("bound")
    assert m == 1024 and bool(c.mask.all())
    c, b, ncls, h, w, m = dims("stacked")
    per = c.mask.sum(1)
    assert int((per == 0).sum()) >= 3 and int((per > 0).sum()) >= 3 and int(per[0]) == 0
    assert get_case("forward_1025").ind.shape[1] == 1025
    for name in ("partial_wave", "strided_objects", "saturated"):
        c = get_case(name)
        live_cells = {(int(b_), int(c.cat[b_, s]), int(c.ind[b_, s])) for b_, s in zip(*np.nonzero(c.mask.numpy()))}
        w = c.hm.shape[3]
        at_live = [abs(float(c.hm[p])) for p in c.saturated if (p[0], p[1], p[2] * w + p[3]) in live_cells]
        at_bg = [abs(float(c.hm[p])) for p in c.saturated if (p[0], p[1], p[2] * w + p[3]) not in live_cells]
        assert {30.0, 100.0} <= set(at_live) and {30.0, 100.0} <= set(at_bg), name
        assert {float(c.hm[p]) for p in c.saturated} == {30.0, -30.0, 100.0, -100.0}
        assert c.lone_tie is not None and c.lone_plain is not None and c.dup_tie is not None, name
        # a live object at cell 0 of class 0, with slots that are not live (ind 0, cat 0) before and after it
        b_ = c.dup_tie[0]
        assert c.mask[b_, 6] and c.ind[b_, 6] == 0 and c.cat[b_, 6] == 0
        assert not c.mask[b_, 0] and not c.mask[b_, 7] and c.ind[b_, 0] == 0 and c.cat[b_, 7] == 0
