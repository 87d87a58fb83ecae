"""GPU parity of `pn_assign_heatmap_cart_sectors_f32` (``ops.assign_heatmap_cart_sectors``): STROBE's per-sector CenterPoint targets against
the reference's own ``voxelize_streaming_cart`` + ``AssignLabel.assign_centerpoint`` (tests/golden/strobe_train.npz) and, for box counts that are
not in the golden, against the host restatement that tests/test_strobe_train_cpu.py holds to the same golden.  The feature maps are 8 x 8,
8 x 4 and 8 x 8 cells: every splat of radius >= 2 is clipped at some border."""
import numpy as np
import pytest
import torch

from tests import strobe_ref as SR
from tests import strobe_train_ref as TR
from tests.test_strobe_train_cpu import check_targets, max_objs_of, samples_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "no GPU visible"
    from partner_amd import hip
    hip.load()
    return torch.device("cuda:0")


def device_targets(dev, samples, nsec, max_objs, cols=9, **kw):
    from partner_amd import ops
    gb, gc, num = TR.padded_batch(samples, cols)
    t = ops.assign_heatmap_cart_sectors(torch.from_numpy(gb).to(dev), torch.from_numpy(gc).to(dev), torch.from_numpy(num).to(dev), TR.CLASSES, max_objs,
                                        nsec, SR.CART_RANGE, SR.CART_VOXEL, kw.pop("osf", TR.osf_of(nsec)), TR.OVERLAP, TR.MIN_RADIUS, **kw)
    torch.cuda.synchronize()
    return tuple(v.cpu().numpy() for v in (t.hm, t.ind, t.mask, t.cat, t.anno))


@pytest.mark.parametrize("nsec", [1, 2, 4])
def test_targets_vs_reference(dev, golden, nsec):
    """exact ind / mask / cat, anno_box at rtol 1e-5 / atol 2e-6, hm at rtol 1e-6 / atol 1e-7 (test_target_assignment_on_device's bounds): a
    set with an empty sample, one with more kept boxes than max_objs, the training set, and the exact cases on the sector borders"""
    g = golden("strobe_train.npz")
    for name in ("mixed", "dense", "train", "exact"):
        got = device_targets(dev, samples_of(name), nsec, max_objs_of(name))
        assert got[0].dtype == np.float32 and got[1].dtype == np.int64 and got[2].dtype == np.uint8 and got[3].dtype == np.int64
        check_targets(got, g, name, nsec)


@pytest.mark.parametrize("nsec", [1, 2, 4])
def test_targets_vs_restatement(dev, nsec):
    """samples of 0 / 1 / 37 / 220 / 300 boxes in one batch (300: more than one pass of the block over the boxes; 220 and 300 overflow
    max_objs = 64 in some sector), ten box columns with the yaw in the last one; outputs that held other values before the call"""
    counts = (0, 1, 37, 220, 300)
    samples = []
    for k, n in enumerate(counts):
        boxes, classes = TR.random_boxes(n, 7000 + 10 * nsec + k)
        wide = np.concatenate([boxes[:, :8], np.full((n, 1), 9.75, np.float32), boxes[:, 8:]], 1)      # a column the entry must not read as the yaw
        samples.append(TR.group_by_class(wide, classes))
    ref = TR.stacked_targets(samples, nsec, 64)
    assert int(ref[2].sum()) > 0 and any(int(TR.sector_keep(samples[4][0], s, nsec).sum()) > 64 for s in range(nsec))
    got = device_targets(dev, samples, nsec, 64, cols=10)
    again = device_targets(dev, samples, nsec, 64, cols=10)
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[1], ref[1])
    np.testing.assert_array_equal(got[3], ref[3])
    np.testing.assert_allclose(got[4], ref[4], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-6, atol=1e-7)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)       # the integer maximum is order independent


def test_refusals(dev):
    from partner_amd import hip, ops
    samples = samples_of("train")
    for nsec in (0, 3, 8, 16):
        with pytest.raises(NotImplementedError, match="nsectors"):
            device_targets(dev, samples, nsec, 8, osf=4)
    with pytest.raises(hip.PartnerHipError, match="at least 9 columns"):
        device_targets(dev, [(b[:, :8], c) for b, c in samples], 4, 8, cols=8)
    with pytest.raises(hip.PartnerHipError, match="no CPU fallback"):
        gb, gc, num = TR.padded_batch(samples)
        ops.assign_heatmap_cart_sectors(torch.from_numpy(gb), torch.from_numpy(gc), torch.from_numpy(num), 10, 8, 4, SR.CART_RANGE, SR.CART_VOXEL, 4)
