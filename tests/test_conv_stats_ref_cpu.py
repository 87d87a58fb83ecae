"""tests/conv_stats_ref.py (the restatement tests/test_hip_conv_stats.py judges the kernels by) pinned to independent formulations
in float64: torch.nn.functional.group_norm, oracle.polar_oracle.rs_norm and oracle.polar_oracle.range_stratified, and an explicit
normalise-then-convolve.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from oracle import polar_oracle as O
from tests import conv_stats_ref as R

F64 = torch.float64
EPS = 1e-5
TOL = 1e-12          # float64 against float64: the formulations differ in the order of a few hundred additions


def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s, k=1.0, m=0.0: (torch.randn(*s, generator=g, dtype=F64) * k + m)  # noqa: E731


def _close(a, b, tol=TOL):
    err = float((a - b).abs().max() / b.abs().max())
    assert err < tol, err


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("per_channel", [False, True])
def test_stats_tables_apply_against_group_norm(per_channel):
    r = _gen(1 + per_channel)
    b, h, w, c = 3, 5, 12, 8
    y, ga, be = r(b, h, w, c, k=1.5, m=0.3), r(c).abs() + 0.5, r(c)
    ref = _nhwc(F.group_norm(_nchw(y), c if per_channel else 1, ga, be, R.f32_eps(EPS)))
    mean, var = R.group_stats(y, c if per_channel else 1, 1)
    assert mean.shape == (b, 1, c if per_channel else 1)
    stat, tab = R.tables(mean, var, EPS, ga, be, c)
    assert stat.shape == (b, 1, mean.shape[2], 2) and tab.shape == (b, 1, c, 2)
    out, out2 = R.apply(y, stat[..., 0], stat[..., 1], ga, be)
    assert out2 is None
    _close(out, ref)
    _close(y * tab[:, :, None, :, 0] + tab[:, :, None, :, 1], ref)             # the affine table says the same
    mul, add = r(h, w, c), r(h, w, c)
    out, out2 = R.apply(y, stat[..., 0], stat[..., 1], ga, be, R.ACT_RELU, mul, add)
    _close(out, torch.relu(ref))
    _close(out2, torch.relu(ref) * mul + add)


@pytest.mark.parametrize("strata", [2, 4])
def test_stats_tables_apply_against_rs_norm(strata):
    r = _gen(10 + strata)
    b, h, w, c = 2, 3, 8 * strata, 12
    y = r(b, h, w, c, k=1.5, m=0.3)
    y[:, :, 8:16] += 3.0                                                       # one stratum stands apart
    ga, be = r(strata, c).abs() + 0.5, r(strata, c)
    ref = _nhwc(O.rs_norm(_nchw(y), ga.reshape(-1), be.reshape(-1), 1, strata, R.f32_eps(EPS)))
    mean, var = R.group_stats(y, 1, strata)
    assert mean.shape == (b, strata, 1)
    stat, tab = R.tables(mean, var, EPS, ga, be, c)
    out, _ = R.apply(y, stat[..., 0], stat[..., 1], ga, be)
    _close(out, ref)
    t = tab[:, None, :, None].expand(b, h, strata, w // strata, c, 2).reshape(b, h, w, c, 2)
    _close(y * t[..., 0] + t[..., 1], ref)
    _close(R.norm_on_load(y, tab, strata), torch.relu(ref))


@pytest.mark.parametrize("strata", [2, 4, 8])
def test_range_stratified_conv_and_norm_against_the_oracle(strata):
    """conv_out(range_strata) + the statistics per (sample, stratum) with gamma / beta row z in table slot z, against the oracle's
    formulation (halo columns stacked on the channels, grouped convolution, GroupNorm with one group per stratum)"""
    r = _gen(20 + strata)
    b, h, w, cin, cout = 2, 4, 6 * strata, 5, 7
    x = r(b, h, w, cin, k=1.5, m=0.3)
    sd = {"conv.0.weight": r(strata * cout, cin, 3, 3, k=0.3), "conv.0.bias": r(strata * cout),
          "conv.1.weight": r(strata * cout).abs() + 0.5, "conv.1.bias": r(strata * cout)}
    ref = _nhwc(O.range_stratified(sd, "", _nchw(x), ngroups=strata))
    y = R.conv_out(x, sd["conv.0.weight"], None, sd["conv.0.bias"], 1, 1, range_strata=strata)
    assert y.shape == (b, h, w, cout)
    mean, var = R.group_stats(y, 1, strata)
    ga, be = sd["conv.1.weight"].view(strata, cout), sd["conv.1.bias"].view(strata, cout)
    stat, tab = R.tables(mean, var, EPS, ga, be, cout)
    out, _ = R.apply(y, stat[..., 0], stat[..., 1], ga, be, R.ACT_RELU)
    _close(out, ref)
    _close(R.norm_on_load(y, tab, strata), ref)
    # ... and a plain convolution with scale and shift
    w1, sc, sh = r(cout, cin, 3, 3), r(cout), r(cout)
    ref1 = _nhwc(F.conv2d(_nchw(x), w1, None, 1, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    _close(R.conv_out(x, w1, sc, sh, 1, 1), ref1)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("strata", [1, 2])
def test_norm_on_load_then_convolution_pads_with_zeros(k, strata):
    """norm_on_load + conv_out against normalising the map explicitly and F.conv2d; with beta > 0 a padding pixel that went through
    the table would be relu(B) > 0 and change the border outputs of a 3x3 kernel"""
    r = _gen(30 + k + 2 * strata)
    b, h, w, c, cout = 2, 3, 8, 8, 4
    x = r(b, h, w, c, k=1.5, m=0.3)
    ga, be = r(strata, c).abs() + 0.5, r(strata, c).abs() + 0.5
    mean, var = R.group_stats(x, 1, strata)
    _, tab = R.tables(mean, var, EPS, ga, be, c)
    assert bool((tab[..., 1] > 0).any())
    wt, sh = r(cout, c, k, k, k=0.3), r(cout)
    got = R.conv_out(R.norm_on_load(x, tab, strata), wt, None, sh, 1, k // 2)
    normed = torch.relu(O.rs_norm(_nchw(x), ga.reshape(-1), be.reshape(-1), 1, strata, R.f32_eps(EPS)))
    ref = _nhwc(F.conv2d(normed, wt, sh, 1, k // 2))
    _close(got, ref)
    if k == 3:      # the fault the reference must not share: the table applied to the padded map
        xp = F.pad(x, (0, 0, 1, 1, 1, 1))
        tcol = tab[:, :, None].expand(b, strata, w // strata, c, 2).reshape(b, w, c, 2)
        tp = torch.cat([tcol[:, :1], tcol, tcol[:, -1:]], 1)                   # (B, W + 2, C, 2): a padding column takes its neighbour's stratum
        bad = torch.relu(xp * tp[:, None, :, :, 0] + tp[:, None, :, :, 1])
        bad = _nhwc(F.conv2d(_nchw(bad), wt, sh, 1, 0))
        d = (bad - ref).abs()
        assert float(d[:, 1:-1, 1:-1].max()) < 1e-12
        assert min(float(d[:, 0].min()), float(d[:, -1].min()), float(d[:, :, 0].min()), float(d[:, :, -1].min())) > 1e-6


SCHEME = [  # (tile, B, H, W, C, channel_groups, strata, range_strata)
    (3, 1, 5, 24, 20, 1, 1, 0), (1, 2, 4, 24, 64, 1, 1, 0), (4, 3, 2, 16, 32, 1, 1, 0), (5, 1, 5, 24, 64, 1, 1, 0),
    (3, 2, 5, 128, 20, 1, 2, 0), (4, 2, 3, 128, 4, 1, 4, 0), (1, 1, 3, 64, 32, 1, 2, 0),
    (3, 1, 5, 24, 20, 20, 1, 0), (1, 2, 8, 16, 64, 64, 1, 0), (3, 2, 8, 16, 4, 4, 1, 0),
    (3, 2, 3, 128, 16, 1, 1, 4), (1, 1, 3, 64, 16, 16, 1, 2),
]


@pytest.mark.parametrize("case", SCHEME, ids=[str(c) for c in SCHEME])
def test_stats_scheme_f32_is_the_same_statistic(case):
    """the float32 summation scheme gives the float64 statistics of the same map to float32 rounding, for every tile and grouping"""
    tile, b, h, w, c, cg, strata, z = case
    g = torch.Generator().manual_seed(sum(case))
    y = (torch.randn(b, h, w, c, generator=g) * 1.5 + 0.3).float()
    mean, var, raw = R.stats_scheme_f32(y, cg, strata, tile, z)
    m64, v64 = R.group_stats(y.double(), cg, z if z > 1 else strata)
    assert mean.shape == m64.shape and mean.dtype == F64
    _close(mean, m64, 2e-6)
    _close(var, v64, 2e-6)
    assert torch.equal(raw.clamp(min=0), var)
