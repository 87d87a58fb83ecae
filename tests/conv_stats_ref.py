"""Plain torch restatement of the convolution-epilogue statistics family of csrc/conv_mfma.hip: the convolution with its per-channel
affine (plain and range-stratified), the GroupNorm / RSNorm group statistics of its output, the tables conv_stats_finalize_kernel
writes, the normalisation conv_stats_apply_kernel applies, and the normalise-on-load of the NORM_IN tile loader.  Every function is
dtype-generic (it computes in the dtype of its first argument), maps are NHWC.  tests/test_conv_stats_ref_cpu.py pins these to
torch.nn.functional.group_norm and to oracle.polar_oracle; tests/test_hip_conv_stats.py compares the kernels with them in float64.

``stats_scheme_f32`` is no reference: it restates the ORDER in which the kernels add in float32 (per lane down 16 or 32 rows of one
column, then the xor butterfly over the wave, or the join over the tile's wave rows) so that the float32 rounding such a scheme may
show (e32) is known for the very inputs of a test."""
import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU = 0, 1

#        tile: (BM, TM, TC, WN)  block rows, 32-row blocks per wave, columns per wave, wave columns (two wave rows everywhere)
TILES = {1: (128, 2, 64, 2), 3: (64, 1, 32, 2), 4: (64, 1, 32, 1), 5: (64, 1, 32, 4)}


def f32_eps(eps):
    """the epsilon the kernels add: a float argument"""
    return float(np.float32(eps))


def conv_out(x, w, scale, shift, stride=1, pad=1, range_strata=0):
    """x (B, H, W, Cin) -> (B, OH, OW, Cout): convolution, then v * scale + shift per output channel (None: 1 / 0).
    range_strata = Z > 1: w is (Z * Cout, Cin, kh, kw) and stratum z of the width (OW / Z columns) is the convolution of the WHOLE
    map with weight block z (so a stratum sees its neighbours' border columns and zeros at the ends of the map)"""
    dt = x.dtype
    y = F.conv2d(x.permute(0, 3, 1, 2), w.to(dt), None, stride, pad)
    if scale is not None:
        y = y * scale.to(dt).view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.to(dt).view(1, -1, 1, 1)
    y = y.permute(0, 2, 3, 1)
    z = int(range_strata)
    if z > 1:
        b, oh, ow, ct = y.shape
        c, step = ct // z, ow // z
        y = torch.cat([y[:, :, k * step:(k + 1) * step, k * c:(k + 1) * c] for k in range(z)], 2)
    return y.contiguous()


def group_stats(y, channel_groups, strata):
    """mean and biased variance of y (B, H, W, C) per (sample, stratum, group), each (B, strata, G): a stratum is a contiguous block
    of W / strata columns, G = 1 (all channels together) or C (every channel on its own)"""
    b, h, w, c = y.shape
    assert w % strata == 0 and channel_groups in (1, c)
    v = y.reshape(b, h, strata, w // strata, c).permute(0, 2, 4, 1, 3)        # (B, S, C, H, W / S)
    v = v.reshape(b, strata, 1, -1) if channel_groups == 1 else v.reshape(b, strata, c, -1)
    mean = v.mean(-1)
    var = ((v - mean[..., None]) ** 2).mean(-1)
    return mean, var


def _rows(p, slots, c):
    """gamma / beta (None, (C,) or (slots, C)) -> (slots, C)"""
    return None if p is None else p.reshape(-1, c).expand(slots, c)


def tables(mean, var, eps, gamma, beta, channels, dtype=None):
    """(mean, rstd) (B, slots, G, 2) and (A, B) (B, slots, C, 2) with A = gamma * rstd, B = beta - mean * A: the kernel's layout
    [b][slot][c].  1 / sqrt runs in the dtype of ``mean``; the tables are then formed in ``dtype`` (default: the same), which is
    what the kernel does with float64 sums and float32 tables"""
    dtype = dtype or mean.dtype
    b, s, g = mean.shape
    rstd = (1.0 / torch.sqrt(var + f32_eps(eps))).to(dtype)
    mean = mean.to(dtype)
    ga = torch.ones(s, channels, dtype=dtype) if gamma is None else _rows(gamma.to(dtype), s, channels)
    be = torch.zeros(s, channels, dtype=dtype) if beta is None else _rows(beta.to(dtype), s, channels)
    a = ga[None] * rstd.expand(b, s, channels)
    bb = be[None] - mean.expand(b, s, channels) * a
    return torch.stack([mean, rstd], -1), torch.stack([a, bb], -1)


def _act(v, act):
    return torch.relu(v) if act == ACT_RELU else v


def apply(y, mean, rstd, gamma, beta, act=ACT_NONE, mul=None, add=None):
    """out = act((y - mean) * rstd * gamma + beta) with mean / rstd (B, S, G) and gamma / beta (S, C) (or (C,), or None);
    out2 = out * mul + add with mul / add (H, W, C), None without them"""
    dt = y.dtype
    b, h, w, c = y.shape
    s = mean.shape[1]
    step = w // s
    spread = lambda t: t.to(dt).expand(b, s, c)[:, None, :, None, :].expand(b, h, s, step, c).reshape(b, h, w, c)  # noqa: E731
    ga = torch.ones(s, c, dtype=dt) if gamma is None else _rows(gamma.to(dt), s, c)
    be = torch.zeros(s, c, dtype=dt) if beta is None else _rows(beta.to(dt), s, c)
    rows = lambda t: t[None, None, :, None, :].expand(b, h, s, step, c).reshape(b, h, w, c)  # noqa: E731
    out = _act((y - spread(mean)) * spread(rstd) * rows(ga) + rows(be), act)
    out2 = None if mul is None else out * mul.to(dt)[None] + add.to(dt)[None]
    return out, out2


def norm_on_load(x, table, strata):
    """relu(x * A + B) of x (B, H, W, C) with (A, B) = table[b][stratum of the column][c] (table (B, strata, >= C, 2)); the
    convolution that follows pads THIS map with zeros"""
    dt = x.dtype
    b, h, w, c = x.shape
    step = w // strata
    t = table.to(dt)[:, :, :c]                                                 # (B, S, C, 2)
    t = t[:, None, :, None].expand(b, h, strata, step, c, 2).reshape(b, h, w, c, 2)
    return torch.relu(x * t[..., 0] + t[..., 1])


def _butterfly(v):
    """pn::wave_sum over the last axis (64 lanes): v += shfl_xor(v, o) for o = 32, 16, .. 1; lane 0's value"""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def stats_scheme_f32(y32, channel_groups, strata, tile, range_strata=0):
    """the statistics of the float32 map y32 (B, H, W, C) the way the epilogue of conv_body and the fold after it form them:
    float32 sums of v and v * v in the kernel's order -- all-channel groups: one pair per 32-row segment and wave column;
    per-channel groups: one pair per column and block tile -- then the fold over the group's partials in float64,
    mean = S1 / n, var = S2 / n - mean^2.  Rows are the pixels of one z slice in (b, h, w) order (range_strata = Z > 1: the slice
    is stratum z of the width, the groups are (b, z)).  Returns mean, var clamped at 0, and the unclamped var, each (B, slots, G),
    float64"""
    assert y32.dtype == torch.float32
    bm, tm, tc, wn = TILES[tile]
    b, h, w, c = y32.shape
    zdim = range_strata if range_strata > 1 else 1
    assert zdim == 1 or strata == 1
    owsub = w // zdim
    slots = zdim if zdim > 1 else strata
    wsub = owsub // strata
    per_channel = channel_groups > 1
    groups = c if per_channel else 1
    bn = wn * tc
    assert c <= bn and not (per_channel and strata > 1) and (strata == 1 or wsub % 32 == 0)
    assert b == 1 or (h * owsub) % (bm if per_channel else 32) == 0, "a tile / segment would straddle two samples"
    lpc, rpl = 64 // tc, 32 // (64 // tc)
    s1 = torch.zeros(b, slots, groups, dtype=torch.float64)
    s2 = torch.zeros_like(s1)
    m = b * h * owsub
    nmt = -(-m // bm)
    row = torch.arange(nmt * bm).clamp(max=m - 1)
    row_b = row // (h * owsub)
    row_s = (row % owsub) // wsub                                             # stratum inside the slice
    for z in range(zdim):
        v = torch.zeros(nmt * bm, bn, dtype=torch.float32)
        v[:m, :c] = y32[:, :, z * owsub:(z + 1) * owsub].reshape(m, c)
        for q, acc in ((v, s1), (v * v, s2)):
            blk = q.view(nmt * bm // 32, lpc, rpl, wn, tc)
            lane = torch.zeros(nmt * bm // 32, lpc, wn, tc, dtype=torch.float32)
            for r in range(rpl):                                              # one lane, down its rows
                lane = lane + blk[:, :, r]
            lane = lane.permute(0, 2, 1, 3)                                   # (segment, wave column, half, column)
            if not per_channel:
                part = _butterfly(lane.reshape(-1, wn, 64)).double()          # (segment, wave column)
                seg_row = torch.arange(nmt * bm // 32) * 32                   # a segment lies in ONE group: that of its first row
                slot = row_s[seg_row] if zdim == 1 else torch.full_like(seg_row, z)
                acc.view(-1).index_add_(0, row_b[seg_row] * slots + slot, part.sum(1))
            else:
                t = lane.reshape(nmt, 2, tm, wn, lpc, tc)                     # (tile, wave row, 32-row block, ...)
                u = torch.zeros(nmt, 2, wn, lpc, tc, dtype=torch.float32)
                for i in range(tm):
                    u = u + t[:, :, i]
                u = u.sum(3) if lpc == 2 else u[:, :, :, 0]                   # the two halves of a column: one addition
                u = (torch.zeros_like(u[:, 0]) + u[:, 0]) + u[:, 1]           # the two wave rows, in order
                part = u.reshape(nmt, bn)[:, :c].double()                     # (tile, column)
                tile_b = row_b[torch.arange(nmt) * bm]
                acc.view(b, slots, groups)[:, z if zdim > 1 else 0].index_add_(0, tile_b, part)
    n = float(h * wsub * (1 if per_channel else c))
    mean = s1 / n
    raw = s2 / n - mean * mean
    return mean, raw.clamp(min=0.0), raw
